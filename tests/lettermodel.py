"""A plain sequential model of the adaptive models of the coders 'b' and 'u' (what the letter instantiations of
wavelet_gpu_models.hip compute with data-parallel passes under BWTC_HIP_LETTER_MODELS=1), and hand-built cases.

ONE loop over the tasks in coding order.  Every task starts with fresh predictors AND fresh machines: the main
machine at 3 ('b', FSM<6>) or absent ('u': slot 0 always), gaps at 2, integers at 1.  The slot follows from the
task's type and the element's gap flag; a main slot is a saturating counter over 1024, 2048, 3072 that starts at
2048 and is itself the probability of a one; the gap and integer slots are those of 'B'.
w = bit << 15 | (bit ? p : 4096 - p).  Nothing is carried: the state handed in is handed on unchanged, and no w
depends on it.  The walk knows no chunks, no slot space and no maps.

From gmmodel come the packing helpers, the case builder and the inputs (codes, tasks) of its cases, which are the
same for every letter."""
import numpy as np

import gmmodel
from gmmodel import GAPS, INNER, INTS, ROOT

LETTERS = ("b", "u")
MAIN_START = {"b": 3, "u": 0}
_N6 = [[0, 3], [0, 3], [1, 3], [2, 4], [2, 5], [2, 5]]        # FSM<6>: [state][bit]


def counter(p, bit):
    """EvenIntervalPredictor<4>: a step of 1024 towards the bit, within [1024, 3072]."""
    return min(p + 1024, 3072) if bit else max(p - 1024, 1024)


class Walk:
    """Per element: w, slot, the slot's value before it, and the three machines before it (packed mc | gc << 3 |
    ic << 5); state_out = state_in."""


def walk(letter, codes, tasks, state_in=0):
    assert letter in LETTERS
    n = len(codes)
    cl = np.asarray(codes).tolist()
    w, slot, before, states = [0] * n, [0] * n, [0] * n, [0] * n
    six = letter == "b"
    for b, e, ty in np.asarray(tasks).tolist():
        mc, gc, ic = MAIN_START[letter], 2, 1
        q = [2048] * 15
        for i in range(b, e):
            v = cl[i]
            bit, flag = v & 1, v >> 1
            states[i] = mc | gc << 3 | ic << 5
            if ty == ROOT:
                k = mc
            elif ty == GAPS:
                k = 8 + gc
            elif ty == INTS:
                k = 12 + ic
            else:
                k = 8 + gc if flag else mc
            x = q[k]
            if k < 8:
                q[k] = counter(x, bit)
            else:
                f = 100 if k >= 12 else 2
                q[k] = x + (((4096 - f) - x) >> 5) if bit else x - ((x - f) >> 5)
            if six and (ty == ROOT or ty == INNER):
                mc = _N6[mc][bit]                       # also under a gap flag, where the main predictor is left alone
            if ty == GAPS or (ty == INNER and flag):
                gc = gmmodel.next4(gc, bit)
            if ty == INTS:
                ic = gmmodel.next3(ic, bit)
            w[i] = (bit << 15) | (x if bit else 4096 - x)
            slot[i], before[i] = k, x
    r = Walk()
    r.w = np.array(w, np.uint16)
    r.slot = np.array(slot, np.int64)
    r.before = np.array(before, np.int64)
    r.states = np.array(states, np.uint32)
    r.state_out = state_in
    return r


def images(bits):
    """A counter walked over `bits` from each of its three values: the three end values."""
    out = []
    for p in (1024, 2048, 3072):
        for b in np.asarray(bits).tolist():
            p = counter(p, b)
        out.append(p)
    return out


def slot_stream(c, wk, k):
    """The bits of slot k in coding order (a case with ONE task that uses slot k: its chain in slot space)."""
    return (c.codes & 1)[wk.slot == k]


# ---- the hand-built cases ------------------------------------------------------------------------------

SINGLE_LENGTHS = (1, 2, 3, 4, 63, 64, 65, 2047, 2048, 2049, 4097)
TYPE_NAMES = {ROOT: "root", GAPS: "gaps", INNER: "inner", INTS: "ints"}


def _single(ty, n):
    # one task of n elements from element 0 (cut at the grid line of 2048); five root elements behind it, so that every
    # case holds elements of the main model -- without them no w could tell a letter from 'B'
    b = gmmodel._Builder(100 * n + ty)
    b.rnd(ty, n, pf=0.4)
    b.task(ROOT, [1, 0, 0, 1, 1])
    return b.case("single_%s_%d" % (TYPE_NAMES[ty], n), 5, {})


def _meet():
    # tasks that meet at G - 64 ... G + 63 for 128 grid lines G, one meeting per line: every offset of the 64-element
    # piece before the line and of the one after it.  The types cycle, so every task start follows a task that has moved
    # the main machine away from where a start puts it.
    b = gmmodel._Builder(5)
    types = (ROOT, INNER, ROOT, GAPS, INNER, INTS)
    for i, off in enumerate(range(-64, 64)):
        at = (i + 1) * gmmodel.CHUNK + off
        b.rnd(types[i % len(types)], at - b.n, pf=0.3)
    b.rnd(ROOT, 100)
    return b.case("meet_grid", 6, {})


def _tails(ty):
    # chunks of 1, 2, 3, 4, 5 and 100 elements that end at a grid line with their task going on, whose last elements are
    # a flip and then 1 ... 4 equal bits of either value (as many of them as the chunk has room for)
    b = gmmodel._Builder(6 + ty)
    for ln in (1, 2, 3, 4, 5, 100):
        for run in (1, 2, 3, 4):
            for bit in (0, 1):
                edge = b.border(ln + 3)
                b.fill_to(edge - ln)
                head = (b.rng.random(ln) < 0.5).astype(np.uint8)
                head[-min(run, ln):] = bit
                if ln > run:
                    head[-run - 1] = bit ^ 1
                body = np.concatenate([head, b.rng.random(40) < 0.5])
                b.task(ty, body, b.rng.random(body.size) < 0.3)
    return b.case("tails_%s" % TYPE_NAMES[ty], 2, {})


def _inner_gaps():
    b = gmmodel._Builder(9)
    for n, pf in ((5, 0.5), (70, 0.5), (300, 0.9), (2500, 0.5), (5000, 0.2), (64, 1.0), (33, 0.5)):
        b.rnd(INNER, n, pf=pf)
        b.runs(INNER, n, mean=4, pf=pf)
    return b.case("inner_gaps", 1, {})


def _alternating(first, doubled_at=None):
    n = 40000
    bits = ((np.arange(n) + first) & 1).astype(np.uint8)
    if doubled_at is not None:
        bits[doubled_at:] ^= 1                         # element doubled_at repeats the one before it
    b = gmmodel._Builder(0)
    b.task(ROOT, bits)
    return b


DOUBLED_BORDER = 5 * gmmodel.SLOT_CHUNK


def _period6():
    b = gmmodel._Builder(0)
    b.task(ROOT, np.resize(np.array((1, 0, 1, 0, 0, 1), np.uint8), 3 * 6 * gmmodel.SLOT_CHUNK + 5))
    return b.case("period6", 4, {})


def _constant(bit):
    b = gmmodel._Builder(0)
    n = 3 * gmmodel.SLOT_CHUNK + 100
    b.task(ROOT, np.full(n, bit, np.uint8))
    b.task(INNER, np.full(n, bit, np.uint8), np.zeros(n, np.uint8))
    b.task(INNER, np.full(n, bit, np.uint8), (np.arange(n) % 3 == 0))
    return b.case("all_%s" % ("ones" if bit else "zeros"), 0, {})


GM_CASES = gmmodel.CASE_NAMES[:gmmodel.CASE_NAMES.index("scan_nc8193") + 1]
_OWN = {}
for _ty in (ROOT, GAPS, INNER, INTS):
    for _n in SINGLE_LENGTHS:
        _OWN["single_%s_%d" % (TYPE_NAMES[_ty], _n)] = (lambda ty, n: (lambda: _single(ty, n)))(_ty, _n)
_OWN.update({
    "meet_grid": _meet, "tails_root": lambda: _tails(ROOT), "tails_inner": lambda: _tails(INNER), "inner_gaps": _inner_gaps,
    "alt_from_0": lambda: _alternating(0).case("alt_from_0", 3, {}), "alt_from_1": lambda: _alternating(1).case("alt_from_1", 3, {}),
    "alt_doubled_before": lambda: _alternating(0, DOUBLED_BORDER - 1).case("alt_doubled_before", 3, {}),
    "alt_doubled_at": lambda: _alternating(0, DOUBLED_BORDER).case("alt_doubled_at", 3, {}),
    "alt_doubled_after": lambda: _alternating(0, DOUBLED_BORDER + 1).case("alt_doubled_after", 3, {}),
    "period6": _period6, "all_zeros": lambda: _constant(0), "all_ones": lambda: _constant(1),
})
SINGLE_CASES = [k for k in _OWN if k.startswith("single_")]
ALT_CASES = ["alt_from_0", "alt_from_1", "alt_doubled_before", "alt_doubled_at", "alt_doubled_after"]
OWN_CASES = list(_OWN)
CASE_NAMES = OWN_CASES + GM_CASES
_made, _walks = {}, {}


def case(name):
    """The case `name` (a gmmodel.Case: codes, tasks, packed, n), built once."""
    if name in GM_CASES:
        return gmmodel.case(name)
    if name not in _made:
        c = _OWN[name]()
        assert c.name == name, (c.name, name)
        _made[name] = c
    return _made[name]


def case_walk(letter, name):
    """The walk of case `name` under `letter` (computed once, shared by the tests, left unchanged)."""
    if (letter, name) not in _walks:
        c = case(name)
        _walks[(letter, name)] = walk(letter, c.codes, c.tasks, c.state_in)
    return _walks[(letter, name)]
