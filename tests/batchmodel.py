"""The batched suffix sorter's rule (bwtc_amd/csrc/batch_bwt.hip), stated once and executable.

THE RULE

Layout.  Block b has size_b >= 1 bytes; T_b is the reversed block plus one 0 byte, n_b = size_b + 1 suffixes.  The
order wanted is the one bwtc_hip_bwt_block produces: plain lexicographic order of the byte strings T_b[i:], a proper
prefix ranking smaller.  The blocks are placed at a common stride S = 2^k, the smallest power of two with
S >= max n_b, so the block of a position s is s >> k and its suffix is s & (S - 1).  Positions s >= b * S + n_b of a
stride are padding: they are never suffixes, never list entries and never read.

Initial key (63 bits): block id (12) | six characters T_b[i .. i + 5], positions at or past n_b reading 0 (48) |
min(n_b - i, 6) (3).  The length field puts a suffix shorter than six characters before any longer suffix that
shares its zero-padded characters, which gives such a suffix a key of its own: two suffixes of one block with the
same length field below six have the same length, so they are the same suffix.  One stable sort of the
m = sum n_b suffixes by key; the block id on top makes every block a contiguous range of slots, in block order,
block b's from base_b = sum of the earlier blocks' n.  rank[s] is the slot of its group's head.

Round at depth h = 6, 12, 24, ...  The list is the entries of groups with more than one member, in slot order.  The
second key of s is rank[s + h] + 1 when s + h lies below the end of s's own block, else 0; the comparison with the
block's end comes before the read, so the look-up can neither touch padding nor cross into the next block.  Gather
the second keys (all of them from the ranks as the round found them), sort by (rank[s], second key), flag the
sub-group heads, write the new rank[] = slot of the sub-group's head, compact the singletons out.  One word goes to
the host per round, the entries left; the rounds end when the list is empty.

Why second key 0 never ties two suffixes.  Entering the round at depth h every group agrees on its first h
characters, the end of the text counting as a character below all others (the length field, then second key 0).  A
suffix shorter than h therefore met its end inside those h characters, and a suffix tied with it would have to end
at the same place: same block, same length, the same suffix.  So a suffix shorter than the depth is alone before
that depth is reached, only a suffix of length exactly h can get second key 0 in a round, and a block has one such
suffix.  sort_scalar asserts it round by round; tests/test_batchmodel.py runs it exhaustively.

Output, per block, with the single-block transform's conventions: row j of block b is slot base_b + j;
out[j] = T_b[SA[j] - 1]; the row of suffix 0 is lf[0] and its hole takes the character of row n_b - 1; size_b
bytes are written; lf[k] = row of suffix n_b - k * (n_b // n_lf); freqs = the block's byte counts.

Two statements of the rule: sort_scalar, position by position over the strided array with its padding poisoned and
every assertion on (small batches), and sort_batch, the same in numpy over the suffixes alone (the test cases' sizes).
`key_chars` (6 in the product) lets the tests run the rounds on batches that six characters would settle outright.
"""
import numpy as np

KEY_CHARS = 6
MAX_BLOCKS = 4096


def n_lf(size, starting_points):
    """bwtc_hip_n_lf: BWTManager's clamp, then BWTBlock::prepareLFpowers."""
    if size <= 256:
        return 1
    return min(256, max(1, starting_points))


def stride_log2(sizes):
    k = 0
    while (1 << k) < max(sizes) + 1:
        k += 1
    return k


def _texts(blocks):
    return [bytes(bytearray(b))[::-1] + b"\0" for b in blocks]


# ---- the rule, position by position -------------------------------------------------------------------------------
def sort_scalar(blocks, key_chars=KEY_CHARS):
    """-> dict(k, rank: {position: slot}, order: positions in slot order, rounds, active).  Asserts the rule's own
    claims: padding is never read, no look-up leaves its block, second key 0 is alone in its group, and the result
    is a permutation."""
    texts = _texts(blocks)
    K = len(texts)
    assert 1 <= K <= MAX_BLOCKS and all(len(t) >= 2 for t in texts)
    k = stride_log2([len(t) - 1 for t in texts])
    S = 1 << k
    T = [None] * (K * S)                                   # None: padding (reading it fails the arithmetic below)
    for b, t in enumerate(texts):
        T[b * S:b * S + len(t)] = list(t)
    n_of = [len(t) for t in texts]
    real = [b * S + i for b in range(K) for i in range(n_of[b])]

    def key(s):
        b, i = s >> k, s & (S - 1)
        chars = 0
        for j in range(key_chars):
            chars = (chars << 8) | (T[s + j] + 0 if i + j < n_of[b] else 0)
        return (b << (8 * key_chars + 3)) | (chars << 3) | min(n_of[b] - i, key_chars)

    keys = {s: key(s) for s in real}
    order = sorted(real, key=lambda s: keys[s])            # stable: ties stay in position order
    rank = {}
    groups = []                                            # (head slot, members) of the groups still tied
    at = 0
    while at < len(order):
        end = at
        while end < len(order) and keys[order[end]] == keys[order[at]]:
            end += 1
        for s in order[at:end]:
            rank[s] = at
        if end - at > 1:
            groups.append((at, order[at:end]))
        at = end
    active = [sum(len(g) for _, g in groups)]
    rounds, h = 0, key_chars
    while groups:
        def second(s):
            b, i = s >> k, s & (S - 1)
            if i + h >= n_of[b]:
                return 0
            assert (s + h) >> k == b and T[s + h] is not None, "a look-up left its block"
            return rank[s + h] + 1
        seconds = {s: second(s) for _, g in groups for s in g}     # all gathered before any rank is written
        next_groups = []
        for head, members in groups:
            assert sum(1 for s in members if seconds[s] == 0) <= 1, "second key 0 tied two suffixes"
            assert all(rank[s] == head for s in members)
            members = sorted(members, key=lambda s: seconds[s])
            at = 0
            while at < len(members):
                end = at
                while end < len(members) and seconds[members[end]] == seconds[members[at]]:
                    end += 1
                for s in members[at:end]:
                    rank[s] = head + at
                if end - at > 1:
                    next_groups.append((head + at, members[at:end]))
                order[head + at:head + end] = members[at:end]
                at = end
        groups = next_groups
        rounds += 1
        active.append(sum(len(g) for _, g in groups))
        h *= 2
    assert sorted(rank.values()) == list(range(len(real)))
    base = 0
    for b in range(K):                                     # every block is its own range of slots, in block order
        assert sorted(rank[b * S + i] for i in range(n_of[b])) == list(range(base, base + n_of[b]))
        base += n_of[b]
    return {"k": k, "rank": rank, "order": order, "rounds": rounds, "active": active}


# ---- the same over the suffixes alone, in numpy ----------------------------------------------------------------------
class Batch:
    """The blocks' suffixes one block after the other: suffix i of block b is number base_b + i."""

    def __init__(self, blocks):
        self.blocks = [np.ascontiguousarray(np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b, np.uint8)
                       for b in blocks]
        assert 1 <= len(self.blocks) <= MAX_BLOCKS and all(b.size >= 1 for b in self.blocks)
        self.sizes = np.array([b.size for b in self.blocks], np.int64)
        self.n = self.sizes + 1
        self.base = np.concatenate([[0], np.cumsum(self.n)[:-1]])
        self.m = int(self.n.sum())
        self.k = stride_log2(self.sizes.tolist())
        self.T = np.zeros(self.m, np.uint8)
        for b, base in zip(self.blocks, self.base):
            self.T[base:base + b.size] = b[::-1]
        self.blk = np.repeat(np.arange(len(self.blocks)), self.n)
        self.i = np.arange(self.m) - self.base[self.blk]
        self.left = self.n[self.blk] - self.i

    def positions(self):
        """the suffixes' positions in the strided array"""
        return (self.blk << self.k) + self.i


def initial_keys(bt, key_chars=KEY_CHARS):
    """One key per suffix, in position order."""
    pad = np.concatenate([bt.T, np.zeros(key_chars, np.uint8)]).astype(np.uint64)
    q = np.arange(bt.m)
    chars = np.zeros(bt.m, np.uint64)
    for j in range(key_chars):
        chars = (chars << np.uint64(8)) | np.where(j < bt.left, pad[q + j], np.uint64(0))
    return (bt.blk.astype(np.uint64) << np.uint64(8 * key_chars + 3)) | (chars << np.uint64(3)) | \
        np.minimum(bt.left, key_chars).astype(np.uint64)


def _rerank(keys_sorted, slots):
    m = keys_sorted.size
    head = np.concatenate([[True], keys_sorted[1:] != keys_sorted[:-1]])
    head_at = np.maximum.accumulate(np.where(head, np.arange(m), 0))
    single = head & np.concatenate([head[1:], [True]])
    return slots[head_at], ~single


def sort_batch(bt, key_chars=KEY_CHARS, check=False):
    """-> (rank by suffix number, rounds, active)."""
    keys = initial_keys(bt, key_chars)
    order = np.argsort(keys, kind="stable")
    rank = np.empty(bt.m, np.int64)
    new, stays = _rerank(keys[order], np.arange(bt.m))
    rank[order] = new
    sfx, slots = order[stays], np.arange(bt.m)[stays]
    active, rounds, h = [int(sfx.size)], 0, key_chars
    while sfx.size:
        inside = bt.left[sfx] > h                            # s + h below the end of s's own block, decided first
        second = np.where(inside, rank[np.where(inside, sfx + h, sfx)] + 1, 0)
        if check:
            ended = rank[sfx][second == 0]
            assert np.unique(ended).size == ended.size, "second key 0 tied two suffixes"
        key = (rank[sfx].astype(np.uint64) << np.uint64(32)) | second.astype(np.uint64)
        o = np.argsort(key, kind="stable")
        sfx = sfx[o]
        new, stays = _rerank(key[o], slots)
        rank[sfx] = new
        sfx, slots = sfx[stays], slots[stays]
        rounds += 1
        active.append(int(sfx.size))
        h *= 2
    if check:
        assert (np.sort(rank) == np.arange(bt.m)).all()
    return rank, rounds, active


def transform(blocks, starting_points=8, key_chars=KEY_CHARS, check=False, n_lfs=None):
    """-> dict(k, rounds, active, keys, T, blocks: [(bytes, lf, freqs)])."""
    bt = Batch(blocks)
    rank, rounds, active = sort_batch(bt, key_chars, check)
    row = rank - bt.base[bt.blk]
    out = []
    for b, blockb in enumerate(bt.blocks):
        base, n, size = int(bt.base[b]), int(bt.n[b]), int(bt.sizes[b])
        rows = row[base:base + n]
        assert rows.min() == 0 and rows.max() == n - 1
        full = np.zeros(n, np.uint8)
        full[rows[1:]] = bt.T[base:base + n - 1]             # out[j] = T[SA[j] - 1]
        p = int(rows[0])
        if p + 1 < n:
            full[p] = full[n - 1]
        nl = n_lfs[b] if n_lfs is not None else n_lf(size, starting_points)
        lf = np.zeros(nl, np.uint32)
        lf[0] = p
        x = n // nl
        for kth in range(1, nl):
            lf[kth] = rows[n - kth * x] if n - kth * x < n else 0
        out.append((full[:size].copy(), lf, np.bincount(blockb, minlength=256).astype(np.uint32)))
    return {"k": bt.k, "rounds": rounds, "active": active, "blocks": out, "suffixes": bt.m}


def keys_and_text(blocks):
    """What bwtc_hip_test_batch_keys returns: (T, keys, counts)."""
    bt = Batch(blocks)
    counts = np.stack([np.bincount(b, minlength=256).astype(np.uint32) for b in bt.blocks])
    return bt.T, initial_keys(bt), counts
