"""A plain sequential model of the 'B' coder's adaptive models (what wavelet_gpu_models.hip computes
with data-parallel passes), the meaning of what every pass must leave, and hand-built cases that reach
the passes' edges.

The reference is ONE loop over the tasks in coding order: three state machines (the main one carried from
task to task, gaps reset to 2 and integers to 1 at every task start), fifteen predictors fresh per task,
w = bit << 15 | probability of the coded bit.  It knows no chunks, no slot space and no brackets.  What
the passes must leave is then stated from that walk's per-element record (slot, value before): the state
at a chunk's start, the counts per chunk and slot, the stable gather of the bits by (slot, task, order),
the true predictor value at every position of that gather.  The "honest bracket" -- the images of the two
extreme start values over the 256 positions before a slot-chunk border -- shows, without the device, that
a case keeps a bracket open where it says it does."""
import numpy as np

ROOT, GAPS, INNER, INTS = 0, 1, 2, 3
CHUNK = 2048          # elements per cell of the packed stream: tasks are cut along this grid
SLOT_CHUNK = 2048     # slot-space positions per slot-chunk
WARM = 256
SAMPLE = 32
SLOTS = 15


def slot_floor(k):
    return 100 if k >= 12 else 2


def slot_delay(k):
    return 4 if k in (0, 7) else 5


def slot_init(k):
    return 2400 - 100 * k if k < 4 else 1996 - 100 * (k - 4) if k < 8 else 2048


def moved(x, bit, floor, d):
    return x + (((4096 - floor) - x) >> d) if bit else x - ((x - floor) >> d)


def next8(s, bit):
    if bit:
        return (s + 1 if s < 7 else 7) if s >= 4 else 4
    return (s - 1 if s else 0) if s < 4 else 3


def next4(s, bit):
    return (bit << 1) | (s >> 1)


def next3(s, bit):
    return min(s + 1, 2) if bit else max(s - 1, 0)


_N8 = [[next8(s, b) for b in (0, 1)] for s in range(8)]
_N4 = [[next4(s, b) for b in (0, 1)] for s in range(4)]
_N3 = [[next3(s, b) for b in (0, 1)] for s in range(3)]
_FLOOR = [slot_floor(k) for k in range(SLOTS)]
_DELAY = [slot_delay(k) for k in range(SLOTS)]
_INIT = [slot_init(k) for k in range(SLOTS)]


class Walk:
    """The sequential walk's record: per element w, slot, predictor value before and after, and the three
    machines before it (packed mc | gc << 3 | ic << 5); state_out = the main machine after the block."""


def walk(codes, tasks, state_in):
    n = len(codes)
    cl = np.asarray(codes).tolist()
    w, slot, before, after, states = [0] * n, [0] * n, [0] * n, [0] * n, [0] * n
    mc = state_in
    for b, e, ty in np.asarray(tasks).tolist():
        gc, ic = 2, 1
        q = list(_INIT)
        for i in range(b, e):
            v = cl[i]
            bit, flag = v & 1, v >> 1
            states[i] = mc | gc << 3 | ic << 5
            if ty == ROOT:
                k = mc
                mc = _N8[mc][bit]
            elif ty == GAPS:
                k = 8 + gc
                gc = _N4[gc][bit]
            elif ty == INTS:
                k = 12 + ic
                ic = _N3[ic][bit]
            else:
                k = 8 + gc if flag else mc
                mc = _N8[mc][bit]               # the main machine also moves under a gap
                if flag:
                    gc = _N4[gc][bit]
            x = q[k]
            y = x + (((4096 - _FLOOR[k]) - x) >> _DELAY[k]) if bit else x - ((x - _FLOOR[k]) >> _DELAY[k])
            q[k] = y
            w[i] = (bit << 15) | (x if bit else 4096 - x)
            slot[i], before[i], after[i] = k, x, y
    r = Walk()
    r.w = np.array(w, np.uint16)
    r.slot = np.array(slot, np.int64)
    r.before = np.array(before, np.int64)
    r.after = np.array(after, np.int64)
    r.states = np.array(states, np.uint32)
    r.state_out = mc
    return r


def end_states(codes, tasks):
    """The main machine after the block from each of the eight states it can start in."""
    cl = np.asarray(codes).tolist()
    st = list(range(8))
    for b, e, ty in np.asarray(tasks).tolist():
        if ty == ROOT or ty == INNER:
            for i in range(b, e):
                bit = cl[i] & 1
                st = [_N8[s][bit] for s in st]
    return st


def machines_over(codes, b, e, ty):
    """The three machines walked over elements [b, e) of a task of type ty from every start state: the images of the
    main states 0..7, of the gap states 0..3 and of the integer states 0..2 (the machines do not look at each other)."""
    m8, m4, m3 = list(range(8)), list(range(4)), list(range(3))
    for v in np.asarray(codes[b:e]).tolist():
        bit, flag = v & 1, v >> 1
        if ty == ROOT or ty == INNER:
            m8 = [_N8[s][bit] for s in m8]
        if ty == GAPS or (ty == INNER and flag):
            m4 = [_N4[s][bit] for s in m4]
        if ty == INTS:
            m3 = [_N3[s][bit] for s in m3]
    return m8, m4, m3


def map_apply(m, st):
    """mapApply of wavelet_gpu_models.hpp: the 38-bit map m applied to a packed state."""
    m = int(m)
    mc, gc, ic = st & 7, (st >> 3) & 3, (st >> 5) & 3
    return ((m >> (3 * mc)) & 7) | (((m >> (24 + 2 * gc)) & 3) << 3) | (((m >> (32 + 2 * ic)) & 3) << 5)


def popcount(v):
    return bin(int(v)).count("1")


def resolve(x0, mask, L, t):
    """A bracket (value of the lowest candidate x0, mask of surviving increments, base L) resolved with the true start
    value t: None where t lies outside an open bracket."""
    if mask == 0:
        return int(x0)
    off = int(t) - int(L)
    if off < 0 or off > 31:
        return None
    return int(x0) + popcount(int(mask) & ((1 << off) - 1))


def pack_codes(codes):
    """16 elements per 32-bit word, element i in bits 2 (i % 16) .. of word i / 16."""
    c = np.asarray(codes, np.uint32)
    pad = (-c.size) % 16
    c = np.concatenate([c, np.zeros(pad, np.uint32)]).reshape(-1, 16)
    return (c << (2 * np.arange(16, dtype=np.uint32))).sum(1).astype(np.uint32)


def unpack_codes(packed, n):
    p = np.asarray(packed, np.uint32)
    return ((p[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)[:n].astype(np.uint8)


def cut_chunks(tasks):
    """(begin, end, task | first << 31) per chunk: every task cut along the grid of CHUNK elements; first chunk per task."""
    out, first = [], []
    for t, (b, e, _) in enumerate(np.asarray(tasks).tolist()):
        first.append(len(out))
        a = b
        while a < e:
            z = min(e, (a // CHUNK + 1) * CHUNK)
            out.append((a, z, t | ((1 << 31) if a == b else 0)))
            a = z
    return np.array(out, np.uint32).reshape(-1, 3), np.array(first, np.int64)


class Expect:
    """What every pass must leave, from the walk's record."""

    def __init__(self, codes, tasks, wk):
        codes = np.asarray(codes, np.uint8)
        tasks = np.asarray(tasks, np.int64).reshape(-1, 3)
        n, nt = codes.size, tasks.shape[0]
        self.n, self.nt = n, nt
        self.chunks, self.first_chunk = cut_chunks(tasks)
        nc = self.nc = self.chunks.shape[0]
        cb = self.chunks[:, 0].astype(np.int64)
        self.cstate = wk.states[cb].copy()
        # counts per (slot, chunk); base = their exclusive prefix in slot-major order, and the total
        chunk_of = np.repeat(np.arange(nc), (self.chunks[:, 1] - self.chunks[:, 0]).astype(np.int64))
        self.cnt = np.zeros((SLOTS, nc), np.int64)
        np.add.at(self.cnt, (wk.slot, chunk_of), 1)
        flat = self.cnt.reshape(-1)
        self.base = np.concatenate([[0], np.cumsum(flat)]).astype(np.uint32)
        self.sb = np.concatenate([self.base[:-1].reshape(SLOTS, nc)[:, self.first_chunk].reshape(-1), [n]]).astype(np.uint32)
        # the stable gather: slot-major, then coding order (tasks are in coding order)
        self.order = np.argsort(wk.slot, kind="stable")
        bits = (codes & 1)[self.order]
        words = np.zeros((n // 32 + 16) * 32, np.uint8)
        words[:n] = bits
        self.gbits = bits.astype(np.int64)
        self.sbits = (words.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(1).astype(np.uint32)
        self.val = wk.before[self.order]              # the true predictor value at every slot-space position
        self.val_after = wk.after[self.order]
        self.slot_at = wk.slot[self.order]
        self.nsc = (n + SLOT_CHUNK - 1) // SLOT_CHUNK
        self.sstart = self.val[::SLOT_CHUNK].astype(np.uint16)
        # chains: the non-empty streams' starts
        sb = self.sb.astype(np.int64)
        self.chain_starts = np.unique(sb[:-1][sb[1:] > sb[:-1]])

    def chain_start_of(self, p):
        return int(self.chain_starts[np.searchsorted(self.chain_starts, p, side="right") - 1])

    def starts_inside(self, j):
        """Chains that start strictly inside slot-chunk j."""
        p0, p1 = j * SLOT_CHUNK, min((j + 1) * SLOT_CHUNK, self.n)
        cs = self.chain_starts
        return int(np.count_nonzero((cs > p0) & (cs < p1)))

    def bracket(self, j):
        """The honest bracket at the border before slot-chunk j: (L, width); width 0 = known exactly (the chain starts
        at most WARM positions before the border)."""
        p0 = j * SLOT_CHUNK
        s0 = self.chain_start_of(p0)
        k = int(self.slot_at[p0])
        if p0 - s0 <= WARM:
            return int(self.val[p0]), 0
        lo, hi = _FLOOR[k], 4096 - _FLOOR[k]
        for b in self.gbits[p0 - WARM:p0].tolist():
            lo, hi = moved(lo, b, _FLOOR[k], _DELAY[k]), moved(hi, b, _FLOOR[k], _DELAY[k])
        return lo, hi - lo

    def candidate_images(self, j):
        """For an open bracket at border j with no chain starting inside the slot-chunk: the honest images of the
        candidates L .. L + width at the chunk's end."""
        L, width = self.bracket(j)
        p0, p1 = j * SLOT_CHUNK, min((j + 1) * SLOT_CHUNK, self.n)
        k = int(self.slot_at[p0])
        x = np.arange(L, L + width + 1, dtype=np.int64)
        f, d = _FLOOR[k], _DELAY[k]
        for b in self.gbits[p0:p1].tolist():
            x = x + (((4096 - f) - x) >> d) if b else x - ((x - f) >> d)
        return x


# ---- the hand-built cases ------------------------------------------------------------------------------

class Case:
    def __init__(self, name, codes, tasks, state_in, edge):
        self.name, self.state_in, self.edge = name, state_in, edge
        self.codes = np.ascontiguousarray(codes, np.uint8)
        self.tasks = np.ascontiguousarray(tasks, np.uint32).reshape(-1, 3)
        self.n = int(self.codes.size)
        self.packed = pack_codes(self.codes)
        self._walks = {}
        self._expect = {}

    def walk(self, state_in=None):
        s = self.state_in if state_in is None else state_in
        if s not in self._walks:
            self._walks[s] = walk(self.codes, self.tasks, s)
        return self._walks[s]

    def expect(self, state_in=None):
        s = self.state_in if state_in is None else state_in
        if s not in self._expect:
            self._expect[s] = Expect(self.codes, self.tasks, self.walk(s))
        return self._expect[s]


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.codes, self.tasks, self.n, self.turn = [], [], 0, 0

    def task(self, ty, bits, flags=None):
        bits = np.asarray(bits, np.uint8) & 1
        assert bits.size > 0
        fl = np.zeros_like(bits) if (flags is None or ty != INNER) else (np.asarray(flags, np.uint8) & 1)
        self.codes.append(bits | (fl << 1))
        self.tasks.append((self.n, self.n + bits.size, ty))
        self.n += int(bits.size)

    def rnd(self, ty, n, p=0.5, pf=0.3):
        self.task(ty, self.rng.random(n) < p, self.rng.random(n) < pf)

    def runs(self, ty, n, mean=40, pf=0.3):
        """bits in runs of geometric length"""
        k = n + 2
        lens = self.rng.geometric(1.0 / mean, k)
        bits = np.repeat((np.arange(k) + int(self.rng.integers(0, 2))) & 1, lens)[:n]
        self.task(ty, bits, self.rng.random(n) < pf)

    def fill_to(self, pos, most=700):
        """filler tasks of all four types up to element `pos`"""
        while self.n < pos:
            m = int(min(pos - self.n, self.rng.integers(1, most)))
            self.rnd(self.turn & 3, m, p=float(self.rng.choice([0.5, 0.9, 0.1])))
            self.turn += 1

    def border(self, room):
        """the first cell border with at least `room` elements before it"""
        return (self.n + room + CHUNK - 1) // CHUNK * CHUNK

    def case(self, name, state_in, edge):
        return Case(name, np.concatenate(self.codes), self.tasks, state_in, edge)


def _tiny_ladder():
    b = _Builder(1)
    for n in (1, 2, 3, 4, 5):
        for pat in range(1 << n):
            for ty in (ROOT, GAPS, INNER, INTS):
                bits = [(pat >> i) & 1 for i in range(n)]
                b.task(ty, bits, b.rng.random(n) < 0.4)
    return b.case("tiny_ladder", 5, {"chunk_lens": {1, 2, 3, 4, 5}, "root_last4": 16, "inner_last4": 16, "nt": 248})


def _inner_tails():
    # INNER chunks of 31, 32, 33 and 100 elements that end at a cell border with their task going on (only then does the
    # gap part of the chunk's map reach anything), by the gap flags among the last 32 elements
    b = _Builder(2)
    for n in (31, 32, 33, 100):
        for where in ((), (0,), (31,), (0, 31), (5,), (3, 17), (0, 32), (31, 40), (7, 33, 50)):
            where = [p for p in where if p < n]
            edge = b.border(n + 3)
            b.fill_to(edge - n)
            flags = np.zeros(n + 60, np.uint8)
            for p in where:
                flags[n - 1 - p] = 1                 # tail position p = element end - 1 - p
            flags[n:] = b.rng.random(60) < 0.6
            b.task(INNER, b.rng.random(n + 60) < 0.5, flags)
    return b.case("inner_tails", 3, {"chunk_lens": {31, 32, 33}, "inner_tail_flags": {0, 1, 2}, "inner_flag_at": {0, 31},
                                     "inner_older_flag_only": 4})


def _alt(n, first):
    return (np.arange(n) + first) & 1


def _ints_tails():
    # INTS chunks that end at a cell border with their task going on: first chunks of 2, 63, 64, 65 and 200 alternating
    # bits, and whole middle chunks (entered in integer state 2, 1 and 0) whose bits alternate over the last 63 / 64 / 65
    # elements and beyond, the latest equal pair at tail positions 62/63, 63/64, 64/65, or nowhere
    b = _Builder(3)
    for n in (2, 63, 64, 65, 200):
        for first in (0, 1):
            edge = b.border(n + 3)
            b.fill_to(edge - n)
            b.task(INTS, np.concatenate([_alt(n, first), b.rng.random(50) < 0.5]))
    for lead in ((1, 1), (0, 0), (1, 0)):
        for pair in (None, 61, 62, 63, 64, 200):
            for last in (0, 1):
                edge = b.border(len(lead) + 3)
                b.fill_to(edge - len(lead))
                mid = _alt(CHUNK, last + 1)                     # the chunk's last bit = last
                if pair is not None:
                    mid[:CHUNK - 1 - pair] ^= 1                 # elements pair and pair + 1 from the end are equal
                b.task(INTS, np.concatenate([lead, mid, b.rng.random(40) < 0.5]))
    return b.case("ints_tails", 0, {"chunk_lens": {2, 63, 64, 65, 200}, "ints_alt_lens": {2, 63, 64, 65, 200, 2048},
                                    "ints_pair_at": {61, 62, 63, 64}, "ints_mid_start": {0, 1, 2}})


def _alignments():
    # 64 tasks of 67 elements: a chunk starts at every residue mod 64, every type ends at every place of a packed word;
    # then the four shapes of the emit pass: one whole aligned piece of 64, whole words without a whole piece, inside one
    # word, ragged at both ends
    b = _Builder(4)
    for i in range(64):
        ty = (INTS, ROOT, INNER, GAPS)[(i // 16) % 4]
        b.runs(ty, 67, mean=5)
    b.fill_to((b.n + 63) // 64 * 64)
    b.rnd(ROOT, 64)
    b.rnd(GAPS, 16)
    b.rnd(INNER, 32)
    b.rnd(INTS, 5)
    b.rnd(ROOT, 7)
    b.rnd(INNER, 90)
    return b.case("alignments", 6, {"begin_mod64": 64, "ints_end_mod16": 16, "root_end_mod16": 16, "inner_end_mod16": 16,
                                    "emit_shapes": {"piece", "words", "inword", "ragged"}, "tail_words": {4, 5}})


def _scan_case(nc, seed, long_at=None):
    # tasks of 1-3 elements that never cross a cell border, so every task is one chunk; most are GAPS or INTS (they leave
    # the main machine alone); ROOT tasks of 1-3 EQUAL bits -- maps that depend on the state they meet -- at the first and
    # last chunk of a thread's eight and of a tile of 8192.  long_at: a long INNER task whose first chunk is chunk
    # long_at, so that its continuation chunks (bit 31 clear) sit at those places too.
    b = _Builder(seed)
    c = 0
    special = lambda i: i % 8 in (0, 7)
    while c < nc:
        if long_at is not None and c == long_at:
            k = min(4, nc - c - 1)                                    # continuation chunks
            first = CHUNK - b.n % CHUNK
            n = first + (k - 1) * CHUNK + 5 if k > 0 else min(first, 3)
            bits = np.zeros(n, np.uint8)
            bits[:first] = b.rng.random(first) < 0.5
            bits[first:] = int(b.rng.integers(0, 2))                  # the continuation chunks: equal bits
            if k > 0:
                bits[-2:] = (1, 1)
            b.task(INNER, bits, b.rng.random(n) < 0.3)
            c += k + 1 if k > 0 else 1
            continue
        room = CHUNK - b.n % CHUNK
        m = int(min(room, b.rng.integers(1, 4)))
        if special(c):
            b.task(ROOT, np.full(m, int(b.rng.integers(0, 2))))
        else:
            b.rnd((GAPS, INTS, GAPS, INTS, INNER)[int(b.rng.integers(0, 5))] if b.rng.random() < 0.97 else ROOT, m)
        c += 1
    return b


def _scan(nc, seed, long_at=None):
    b = _scan_case(nc, seed, long_at)
    edge = {"nc": nc, "nc_exact": nc}
    if nc >= 8:
        edge["root_equal_at_thread_edges"] = {0, 7} if nc != 9 else {0}
    if nc > 8192:
        edge["root_equal_at_tile_edges"] = {0, 8191}
    if long_at is not None:
        edge["continuation_at_thread_edges"] = {0, 7}
        if nc > 8192:
            edge["continuation_at_tile_edges"] = {0, 8191}
    return b.case("scan_nc%d" % nc, nc % 8, edge)


def _streams(nc, seed):
    # nc one-chunk tasks: 15 nc + 1 words go through the exclusive scan (4096 = its last one-tile size).  Many tasks use
    # a single slot (one element), which leaves runs of empty streams for streamAt's search
    b = _Builder(seed)
    for i in range(nc):
        if i % 3 == 0:
            b.rnd(i & 3, 1)
        else:
            b.rnd(int(b.rng.integers(0, 4)), int(b.rng.integers(1, 8)), p=0.8)
    return b.case("streams_nc%d" % nc, 2, {"nc_exact": nc, "nt": nc, "single_slot_tasks": nc // 3, "empty_stream_run": 8})


def _few_tasks(nt, seed):
    b = _Builder(seed)
    for i in range(nt):
        if i % 4 == 1:
            b.rnd(ROOT, 1)
        else:
            b.runs(i & 3, int(b.rng.integers(20, 400)), mean=6)
    return b.case("streams_nt%d" % nt, 1, {"nt_exact": nt, "single_slot_tasks": 4})


def _partition_words():
    # slot 7 alone (ROOT tasks of ones met in state 7): contributions of 32, 1, 31, 33, 64 bits put a chunk's first
    # position at bits 0, 0, 1, 0, 1 ... of a word; then several one-bit tasks inside one word; then a mix of all types
    b = _Builder(7)
    for n in (32, 1, 31, 33, 64, 31, 1, 1, 1, 1, 30, 64, 33, 1, 31, 32):
        b.task(ROOT, np.ones(n, np.uint8))
    for i in range(120):
        ty = int(b.rng.integers(0, 4))
        n = int(b.rng.choice([1, 1, 2, 3, 31, 32, 33, 64, 65, 100]))
        b.runs(ty, n, mean=int(b.rng.choice([2, 30])))
    return b.case("partition_words", 7, {"contributions": {0, 1, 31, 32, 33, 64}, "first_bit": {0, 1, 31}, "chunks_in_word": 3,
                                         "last_word_partial": 1, "P_mod32": {31, 0, 1}, "a0_gt_s0": 1, "a0_le_s0": 1})


def _lines(nc, seed):
    # one-chunk tasks for the lines form of the partition pass: 128 chunks per workgroup; a workgroup's stretch of a slot
    # is empty, one word, two words
    b = _Builder(seed)
    for i in range(nc):
        ty = (GAPS, INTS, ROOT, INNER)[int(b.rng.integers(0, 4))] if i < 128 else (GAPS if i % 2 else INTS)
        room = CHUNK - b.n % CHUNK
        b.rnd(ty, int(min(room, b.rng.integers(1, 4))), p=0.7)
    return b.case("lines_nc%d" % nc, 4, {"nc_exact": nc, "stretch_words": {0, 1, 2}})


_PERIOD6 = (0, 0, 1, 0, 1, 0)
_PERIOD8 = (0, 1, 1, 0, 1, 0, 0, 1)


def _chain_bits(prefix, pattern, n):
    return np.concatenate([np.array(prefix, np.uint8), np.resize(np.array(pattern, np.uint8), n - len(prefix))])


def _gaps_for_slot11(chain):
    """A GAPS task's bits that give slot 11 (the last two bits were ones) exactly `chain`: after a zero, two ones lead back."""
    out = [1]
    for c in chain.tolist():
        out += [c] if c else [0, 1, 1]
    return np.array(out, np.uint8)


def _root_for_slot7(chain):
    """A ROOT task's bits that give slot 7 (main state 7) exactly `chain`: after a zero, four ones lead back."""
    out = [1, 1, 1, 1]
    for c in chain.tolist():
        out += [c] if c else [0, 1, 1, 1, 1]
    return np.array(out, np.uint8)


def _open_brackets():
    # long chains that keep their bracket open: constant bits (the widest bracket, 2^d - 1; the true value at its lowest
    # candidate for ones and at its highest for zeros), period 3, alternating, and the period-6 and period-8 patterns of
    # integer tasks whose true value lies strictly inside.  Every task is longer than a slot-chunk and WARM.
    # For the main and gap slots no periodic ELEMENT pattern from a fresh task was found that does the same; a search over
    # the bits of ONE chain (a prefix of up to 8 bits, then a period of up to 8) found some: prefix 0,0,1,1,1,1,0,0 then
    # 0,1,1,0 for (floor 2, delay 5) from 2048 -- width 2, the true value in the middle -- and prefix 0,0,1,0,0,0 then
    # 0,1,0 for (floor 2, delay 4) from slot 7's 1696 -- width 3.  The last two tasks feed slot 11 and slot 7 those bits.
    b = _Builder(8)
    n = 2 * SLOT_CHUNK + 700
    for ty in (ROOT, GAPS, INTS):
        for bit in (1, 0):
            b.task(ty, np.full(n, bit, np.uint8))
    b.task(INNER, np.ones(n, np.uint8), np.ones(n, np.uint8))
    b.task(INNER, np.zeros(n, np.uint8), np.zeros(n, np.uint8))
    for pat in (_PERIOD6, _PERIOD8, (0, 0, 1), (0, 1)):
        b.task(INTS, np.resize(np.array(pat, np.uint8), 3 * n))
        b.task(GAPS, np.resize(np.array(pat, np.uint8), 3 * n))
        b.task(ROOT, np.resize(np.array(pat, np.uint8), 3 * n))
    b.task(GAPS, _gaps_for_slot11(_chain_bits((0, 0, 1, 1, 1, 1, 0, 0), (0, 1, 1, 0), n)))
    b.task(ROOT, [0])                                 # the main state is below 4 now: the next four ones land in slots 3 to 6
    b.task(ROOT, _root_for_slot7(_chain_bits((0, 0, 1, 0, 0, 0), (0, 1, 0), n)))
    return b.case("open_brackets", 4, {"inside_2_5": 1, "inside_2_4": 1, "bracket_2_4": {(15, "low"), (15, "top")}, "bracket_2_5": {(31, "low"), (31, "top")},
                                       "bracket_100_5": {(31, "low"), (31, "top")}, "inside_100_5": 1,
                                       "skip_words": 64, "emit_inside": 1})


def _chain_borders():
    # integer tasks of zeros only: one element in slot 13, the rest in slot 12, so the chains of slot 12 lie where the
    # lengths put them: a chain starts 256 positions before a border (the exact walk), 257 before one (the bracket),
    # exactly at one, and in the middle of a word, on a word border and several times inside one word
    b = _Builder(9)
    for m in (1792, 2047, 2305, 2048 + 300):          # chains of slot 12 at 0, 1792, 3839, 6144
        b.task(INTS, np.zeros(m + 1, np.uint8))
    for m in (5, 3, 1, 2, 24, 32, 7):                  # chains inside one word, then one on a word border
        b.task(INTS, np.zeros(m + 1, np.uint8))
    b.task(INTS, np.zeros(1, np.uint8))               # a task with an EMPTY stream in slot 12
    b.task(INTS, np.zeros(70, np.uint8))
    b.task(INTS, np.ones(40, np.uint8))
    return b.case("chain_borders", 0, {"chain_before_border": {0, 256, 257}, "chains_in_word": 3, "chain_on_word_border": 2,
                                       "chain_inside_word": 4})


def _unsaturated_skip():
    # runs of 64 and more equal bits where the candidates still move (the whole-word shortcut must NOT be taken): a long
    # gaps task of ones, then zeros from shortly before a slot-chunk border on; and the same after saturation
    b = _Builder(10)
    b.task(GAPS, np.concatenate([np.ones(SLOT_CHUNK + 300, np.uint8), np.zeros(600, np.uint8), np.ones(500, np.uint8)]))
    b.task(INTS, np.concatenate([np.zeros(SLOT_CHUNK + 500, np.uint8), np.ones(700, np.uint8), np.zeros(300, np.uint8)]))
    b.task(ROOT, np.concatenate([np.ones(SLOT_CHUNK + 400, np.uint8), np.zeros(400, np.uint8)]))
    return b.case("unsaturated_skip", 7, {"equal_words_moving": 8, "equal_words_moving_open": 1, "skip_words": 8})


def _total(n, seed, name=None):
    # a mix of everything with exactly n coded elements: n sets the number of slot-chunks and the size of the last one
    b = _Builder(seed)
    while b.n < n:
        m = int(min(n - b.n, b.rng.choice([1, 3, 40, 300, 2500, 5000])))
        kind = int(b.rng.integers(0, 3))
        ty = b.turn & 3
        b.turn += 1
        if kind == 0:
            b.rnd(ty, m, p=float(b.rng.choice([0.5, 0.95, 0.05])))
        elif kind == 1:
            b.runs(ty, m, mean=int(b.rng.choice([3, 80])))
        else:
            pat = (_PERIOD6, _PERIOD8, (0, 0, 1), (1,), (0,))[int(b.rng.integers(0, 5))]
            b.task(ty, np.resize(np.array(pat, np.uint8), m), b.rng.random(m) < 0.2)
    nsc = (n + SLOT_CHUNK - 1) // SLOT_CHUNK
    return b.case(name or "total_%d" % n, seed % 8, {"total_exact": n, "nsc_exact": nsc, "last_slot_chunk_exact": n - (nsc - 1) * SLOT_CHUNK})


_CASES = [
    _tiny_ladder, _inner_tails, _ints_tails, _alignments,
    lambda: _scan(1, 11), lambda: _scan(7, 12), lambda: _scan(8, 13), lambda: _scan(9, 14, long_at=6),
    lambda: _scan(8191, 15), lambda: _scan(8192, 16), lambda: _scan(8193, 17), lambda: _scan(16385, 18, long_at=8190),
    lambda: _streams(273, 21), lambda: _streams(274, 22), lambda: _few_tasks(17, 23), lambda: _few_tasks(18, 24),
    _partition_words, lambda: _lines(127, 31), lambda: _lines(128, 32), lambda: _lines(129, 33),
    _open_brackets, _chain_borders, _unsaturated_skip,
    lambda: _total(2047, 41), lambda: _total(2048, 42), lambda: _total(2049, 43),
] + [(lambda r: (lambda: _total(2 * SLOT_CHUNK + r, 50 + r)))(r) for r in (1, 31, 32, 33, 63, 64, 65)] + [
    lambda: _total(15 * SLOT_CHUNK - 100, 61), lambda: _total(16 * SLOT_CHUNK, 62), lambda: _total(16 * SLOT_CHUNK + 40, 63),
    lambda: _total(32 * SLOT_CHUNK + 5, 64),
]
CASE_NAMES = (["tiny_ladder", "inner_tails", "ints_tails", "alignments"] + ["scan_nc%d" % n for n in (1, 7, 8, 9, 8191, 8192, 8193, 16385)] +
              ["streams_nc273", "streams_nc274", "streams_nt17", "streams_nt18", "partition_words", "lines_nc127", "lines_nc128",
               "lines_nc129", "open_brackets", "chain_borders", "unsaturated_skip", "total_2047", "total_2048", "total_2049"] +
              ["total_%d" % (2 * SLOT_CHUNK + r) for r in (1, 31, 32, 33, 63, 64, 65)] +
              ["total_%d" % n for n in (15 * SLOT_CHUNK - 100, 16 * SLOT_CHUNK, 16 * SLOT_CHUNK + 40, 32 * SLOT_CHUNK + 5)])
SCAN_CASES = ["scan_nc%d" % n for n in (1, 7, 8, 9, 8191, 8192, 8193, 16385)]
_made = {}


def case(name):
    """The hand-built case `name` (built once; its walks and expectations are kept with it)."""
    if name not in _made:
        c = _CASES[CASE_NAMES.index(name)]()
        assert c.name == name, (c.name, name)
        _made[name] = c
    return _made[name]


# ---- what a case reaches -------------------------------------------------------------------------------------

def _off_class(off, width):
    return "low" if off == 0 else "top" if off == width else "inside"


def measures(c):
    """What the passes meet in case c, from the model alone (tests/test_gmmodel.py holds every case to its `edge`:
    a number is a least value, `*_exact` an exact one, a set must be contained)."""
    wk, ex = c.walk(), c.expect()
    codes, tasks, chunks = c.codes, c.tasks.astype(np.int64), ex.chunks.astype(np.int64)
    bits, flags = (codes & 1).astype(np.int64), (codes >> 1).astype(np.int64)
    n, nc, nt = c.n, ex.nc, ex.nt
    ctype = tasks[chunks[:, 2] & 0x7FFFFFFF, 2]
    clen = chunks[:, 1] - chunks[:, 0]
    first = (chunks[:, 2] >> 31) == 1
    goes_on = np.concatenate([~first[1:], [False]])            # the chunk's task continues in the next chunk
    m = {"nc": nc, "nc_exact": nc, "nt": nt, "nt_exact": nt, "total_exact": n, "nsc_exact": ex.nsc,
         "last_slot_chunk_exact": n - (ex.nsc - 1) * SLOT_CHUNK, "chunk_lens": set(clen.tolist()),
         "begin_mod64": len(set((chunks[:, 0] % 64).tolist()))}
    last4 = {ROOT: set(), INNER: set()}
    tail_flags, flag_at, older = set(), set(), 0
    alt_lens, pair_at, mid_start, tail_words = set(), set(), set(), set()
    end16 = {ROOT: set(), INNER: set(), INTS: set()}
    shapes = set()
    for ci in range(nc):
        b, e, ty, ln = int(chunks[ci, 0]), int(chunks[ci, 1]), int(ctype[ci]), int(clen[ci])
        if ty in last4 and ln >= 4:
            last4[ty].add(tuple(bits[e - 4:e].tolist()))
        if ty in end16 and ln >= (64 if ty == INTS else 4):
            end16[ty].add(e % 16)
        if ty == INTS and ln >= 64:
            tail_words.add((e - 1) // 16 - (e - 64) // 16 + 1)
        if ty == INNER and ln >= 4 and goes_on[ci]:
            t = min(ln, 32)
            f = flags[e - t:e][::-1]                             # tail position p = element end - 1 - p
            tail_flags.add(min(int(f.sum()), 2))
            flag_at |= {p for p in (0, 31) if p < t and f[p]}
            older += int(f.sum() < 2 and flags[b:e - t].sum() > 0)
        if ty == INTS and goes_on[ci]:
            x = bits[b:e][::-1]
            eq = np.flatnonzero(x[:-1] == x[1:])
            if eq.size == 0:
                alt_lens.add(ln)
            else:
                pair_at.add(int(eq[0]))
                if int(eq[0]) >= 61:
                    alt_lens.add(ln)
            if not first[ci] and ln == CHUNK:
                mid_start.add(int(wk.states[b] >> 5))
        if b % 64 == 0 and ln == 64:
            shapes.add("piece")
        elif b % 16 == 0 and e % 16 == 0 and ln < 64 + (-b) % 64:
            shapes.add("words")
        elif b // 16 == (e - 1) // 16 and ln < 16:
            shapes.add("inword")
        elif b % 16 and e % 16 and ln > 32:
            shapes.add("ragged")
    m.update(root_last4=len(last4[ROOT]), inner_last4=len(last4[INNER]), inner_tail_flags=tail_flags, inner_flag_at=flag_at,
             inner_older_flag_only=older, ints_alt_lens=alt_lens, ints_pair_at=pair_at, ints_mid_start=mid_start,
             tail_words=tail_words, ints_end_mod16=len(end16[INTS]), root_end_mod16=len(end16[ROOT]),
             inner_end_mod16=len(end16[INNER]), emit_shapes=shapes)
    # the state scan: ROOT chunks of 1-3 equal bits and continuation chunks, by their place in a thread's eight and in a tile
    eq_root = np.array([ctype[i] == ROOT and clen[i] <= 3 and len(set(bits[chunks[i, 0]:chunks[i, 1]].tolist())) == 1 for i in range(nc)])
    idx = np.arange(nc)
    m["root_equal_at_thread_edges"] = set((idx[eq_root] % 8).tolist()) & {0, 7}
    m["root_equal_at_tile_edges"] = set((idx[eq_root] % 8192).tolist()) & {0, 8191}
    m["continuation_at_thread_edges"] = set((idx[~first] % 8).tolist()) & {0, 7}
    m["continuation_at_tile_edges"] = set((idx[~first] % 8192).tolist()) & {0, 8191}
    # streams
    used = ex.cnt.reshape(SLOTS, nc)
    per_task = np.zeros((SLOTS, nt), np.int64)
    np.add.at(per_task, (slice(None), chunks[:, 2] & 0x7FFFFFFF), used)
    m["single_slot_tasks"] = int(np.count_nonzero((per_task > 0).sum(0) == 1))
    empty = (per_task.reshape(-1) == 0).astype(np.int64)
    run = best = 0
    for v in empty.tolist():
        run = run + 1 if v else 0
        best = max(best, run)
    m["empty_stream_run"] = best
    # partition
    base = ex.base[:-1].astype(np.int64).reshape(SLOTS, nc)
    m["contributions"] = set(used.reshape(-1).tolist())
    m["first_bit"] = set((base[used > 0] % 32).tolist())
    share = 0
    for k in range(SLOTS):
        live = np.flatnonzero(used[k] > 0)
        if live.size:
            cnt = {}                                             # chunks that put bits into a word (its first or last)
            for i in live.tolist():
                for wd in {int(base[k, i] // 32), int((base[k, i] + used[k, i] - 1) // 32)}:
                    cnt[wd] = cnt.get(wd, 0) + 1
            share = max(share, max(cnt.values()))
    m["chunks_in_word"] = share
    m["last_word_partial"] = int(n % 32 != 0)             # the last slot's last bits leave through the closing OR
    nw = set()
    for c0 in range(0, nc, 128):
        c1 = min(c0 + 128, nc)
        for k in range(SLOTS):
            g0 = int(ex.base[k * nc + c0])
            g1 = int(ex.base[k * nc + c1])
            nw.add(((g1 - 1) // 32 - g0 // 32 + 1) if g1 > g0 else 0)
    m["stretch_words"] = nw
    # brackets at the slot-chunk borders
    br = {(2, 4): set(), (2, 5): set(), (100, 5): set()}
    inside = {(2, 4): 0, (2, 5): 0, (100, 5): 0}
    dist = set()
    open_inside_chunks = set()
    for j in range(ex.nsc):
        p0 = j * SLOT_CHUNK
        k = int(ex.slot_at[p0])
        dist.add(p0 - ex.chain_start_of(p0))
        L, width = ex.bracket(j)
        if width:
            assert width < (1 << _DELAY[k]), (c.name, j, width)
            off = int(ex.val[p0]) - L
            assert 0 <= off <= width
            cls = _off_class(off, width)
            br[(_FLOOR[k], _DELAY[k])].add((width, cls))
            if cls == "inside":
                inside[(_FLOOR[k], _DELAY[k])] += 1
                open_inside_chunks.add(j)
    for (f, d), s in br.items():
        m["bracket_%d_%d" % (f, d)] = s
        m["inside_%d_%d" % (f, d)] = inside[(f, d)]
    m["chain_before_border"] = dist & {0, 256, 257}
    cs = ex.chain_starts
    m["chains_in_word"] = int(np.bincount(cs // 32).max()) if cs.size else 0
    m["chain_on_word_border"] = int(np.count_nonzero(cs % 32 == 0))
    m["chain_inside_word"] = int(np.count_nonzero(cs % 32 != 0))
    # whole words of equal bits in slot space: where the true value stands still, and where it still moves
    nwords = n // 32
    if nwords:
        gw = ex.gbits[:nwords * 32].reshape(-1, 32)
        same = (gw.min(1) == gw.max(1))
        one_chain = np.array([ex.chain_start_of(wd * 32 + 31) <= wd * 32 for wd in np.flatnonzero(same)], bool)
        wd = np.flatnonzero(same)[one_chain]
        still = ex.val[wd * 32] == ex.val_after[wd * 32 + 31]
        m["skip_words"] = int(np.count_nonzero(still))
        m["equal_words_moving"] = int(np.count_nonzero(~still))
        open_chunk = np.array([ex.bracket(int(p // SLOT_CHUNK))[1] > 0 and ex.starts_inside(int(p // SLOT_CHUNK)) == 0 for p in wd * 32], bool)
        m["equal_words_moving_open"] = int(np.count_nonzero(~still & open_chunk)) if wd.size else 0
    else:
        m["skip_words"] = m["equal_words_moving"] = m["equal_words_moving_open"] = 0
    # the emit pass: a chunk's first position P per slot it uses
    P = base[used > 0]
    s0 = ex.sb[:-1].astype(np.int64).reshape(SLOTS, nt)[:, chunks[:, 2] & 0x7FFFFFFF][used > 0]
    a0 = P // SAMPLE * SAMPLE
    m["P_mod32"] = set((P % 32).tolist())
    m["a0_gt_s0"] = int(np.count_nonzero(a0 > s0))
    m["a0_le_s0"] = int(np.count_nonzero(a0 <= s0))
    m["emit_inside"] = int(sum(1 for p, a, s in zip(P.tolist(), a0.tolist(), s0.tolist())
                               if a > s and (a // SLOT_CHUNK) in open_inside_chunks and ex.starts_inside(a // SLOT_CHUNK) == 0))
    return m


def edge_misses(c):
    """The measures of c.edge that the case does not reach (empty = every edge reached)."""
    m = measures(c)
    miss = {}
    for k, want in c.edge.items():
        got = m[k]
        if isinstance(want, set):
            ok = want <= got
        elif k.endswith("_exact"):
            ok = got == want
        else:
            ok = got >= want
        if not ok:
            miss[k] = (want, got)
    return miss
