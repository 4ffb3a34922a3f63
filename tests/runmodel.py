"""The sorter's run rule, stated on its own (no GPU, no library): a plain prefix-doubling suffix sorter that ranks
long runs of one byte in closed form.

T is the text as the sorter sees it; the end of T compares below every byte.  k[s] is the number of positions from
s on that hold T[s].  A group that shares c^h holds exactly the suffixes with k >= h.  Its order: the members whose
run is followed by a smaller byte (or by the end) come first, by ascending k; the others follow, by descending k;
members equal in that come from different runs, share exactly k characters and are ordered by rank[s + k].

  the run step    one round in which a member with k >= h takes the second key (type, k) or (type, n - k) instead
                  of rank[s + h] + 1; the list's depth h is not doubled by it (h_split = h)
  later rounds    a member with k >= h_split looks up rank[s + max(h, k)], every other member rank[s + h]
  the gate        a list without a member with k >= h takes no run step: its rounds are the plain sorter's

sort_suffixes() returns the order and the number of rounds; tests/test_runmodel.py holds it to sorted()."""


def run_lengths(T):
    """k[s] for every s, and the longest run."""
    n = len(T)
    k = [0] * n
    for s in range(n - 1, -1, -1):
        k[s] = k[s + 1] + 1 if s + 1 < n and T[s + 1] == T[s] else 1
    return k, max(k, default=0)


def falling(T, k, s):
    """The run of s is followed by the end of T or by a smaller byte."""
    e = s + k[s]
    return e == len(T) or T[e] < T[s]


def run_key(T, k, s):
    """The run step's second key: one bit of type above a length."""
    n = len(T)
    return (0, k[s]) if falling(T, k, s) else (1, n - k[s])


def run_members(T, depth):
    """The suffixes with k >= depth."""
    k, _ = run_lengths(T)
    return [s for s in range(len(T)) if k[s] >= depth]


def sort_suffixes(T, depth=1, runs=True, step_round=0, others="lookup"):
    """Suffix order of T by prefix doubling from an initial ranking by `depth` characters.

    runs: take the run step, at round `step_round` (if the gate lets it); others: what the members without a long
    run do in that round ("lookup": rank[s + h] as ever, "alone": they keep their group).
    Returns (order, rounds, stepped): stepped is the depth of the run step, or 0."""
    T = bytes(T)
    n = len(T)
    k, longest = run_lengths(T)
    order = sorted(range(n), key=lambda s: T[s:s + depth])
    rank = [0] * n
    groups = []                                  # (first slot, one past the last) of every group still tied

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
        step = runs and not h_split and rounds >= step_round and any(k[order[j]] >= h for lo, hi in groups for j in range(lo, hi))
        pending, nxt = [], []
        for lo, hi in groups:
            members = order[lo:hi]
            keyed = []
            for s in members:
                if step and k[s] >= h:
                    key = (1,) + run_key(T, k, s)
                elif step and others == "alone":
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
        if step:
            h_split = h
        else:
            h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, h_split
