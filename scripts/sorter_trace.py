#!/usr/bin/env python3
"""What the suffix sorter does with a fixed list of small blocks, on one GPU: one JSON line per case, no times.

A line holds the case's name and switch set, the block's size and starting points, SHA-256 of the transformed bytes, the
LF powers, pidx (LF[0]), stats.rounds / route / active_sum / sort_pass_items / finisher_entries / alg_bytes, what
bwtc_hip_period_get and bwtc_hip_steps_get say, and the sorter's debug lines that begin with "runs:", "periods:",
"steps:", "finisher:", "finisher pass", "local pass:" or "shallow groups:", their measured times masked ("took * ms"):
every stretch-length pass (storing or trial, with its period), the vote kernel and each decision, and every finisher
pass and local step with its counts and depths.  Two builds of the library whose traces are equal line for line sorted these blocks by
the same routes, with the same passes in the same order and the same launch-independent counters, to the same bytes:
the check of a change to the sorter's host code that is meant to change nothing.

The blocks come from the tests' own builders (tests/test_gpu_bwt.py, test_gpu_run_ranks.py, test_gpu_period_step.py,
periodcases.py, mixedcases.py), at 4 MiB at most.  A switch is read when a context is made: every switch set gets a
context of its own, one at a time.  The tool itself asserts that the cases between them set every route bit it names in
WANT_BITS, that a block without the long keys (route bit 0 clear) was seen on a 64-bit key plan and on the 32-bit one,
and that the cases with BWTC_HIP_MIXED=1 showed every way the two closed-form steps meet in one block (STEP_SIGHTS) --
equal traces over cases that all took one route would say little.

Usage: scripts/sorter_trace.py [--out FILE]     (BWTC_HIP_LIB=<another build's libbwtc_hip.so> traces that build)"""
import argparse
import hashlib
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mixedcases as mc                   # noqa: E402
import periodcases as pc                  # noqa: E402
import test_gpu_bwt as tb                 # noqa: E402
import test_gpu_period_step as tp         # noqa: E402
import test_gpu_run_ranks as tr           # noqa: E402
from bwtc_amd import hip, synth           # noqa: E402

SMALL = "BWTC_HIP_GRAM_MIN_N=64"          # as the tests do: small blocks through the gram / long-key routes (and a 64-bit key plan)
# Route bit 7 (a finisher pass's lists would not fit) is not wanted: it takes a list of more than 8 Mi entries in a
# context made for exactly the block (m / 64 > cap / 128 + 65536), which no block of 4 MiB has.
# test_wide_finisher_shape_on_blocks_that_are_mostly_tied covers it at 16 MiB.
WANT_BITS = (0, 1, 2, 3, 4, 5, 6, 8)
# The vote count of bwtc_hip_period_get is printed as null for these: the finder counts neighbours of one group in a
# list whose order inside a group the finisher's atomic appends decide, and on the block with the planted run of three
# rare symbols one build's count differs from run to run by a few votes in 2900 (threshold: 256).  Nothing else does.
VOTES_VARY = ("structured_5",)
MIXED = "BWTC_HIP_MIXED=1"
# What the cases with the switch must show between them (main's closing assertion)
STEP_SIGHTS = ("one period step that ranked the runs too", "a period step behind the run step", "no period step after a run step",
               "no period step under a forced period")
# ... and the finisher's own lines: each pass's entries in and out with the hard and shallow counts and depths, what goes on
# to the rounds, the shallow groups' leftovers and the local list's steps, in order
SAID = ("runs:", "periods:", "steps:", "finisher:", "finisher pass", "local pass:", "shallow groups:")
TOOK = re.compile(r"took [0-9.]+ ms")
VOTES = re.compile(r"with [0-9]+ votes")


def switch_rows():
    """The rows of test_sorter_feature_switches_agree, from its parametrize mark."""
    for mark in tb.test_sorter_feature_switches_agree.pytestmark:
        if mark.name == "parametrize":
            return list(mark.args[1])
    raise SystemExit("test_sorter_feature_switches_agree has lost its rows")


def cases():
    """(name, switch set, plan, builder, starting points); plan: "wide" / "32" where the key plan is known by
    construction (BWTC_HIP_GRAM_MIN_N below its default forces 64-bit keys; random bytes and four letters at these sizes
    have too much entropy in four / sixteen characters for them), else None."""
    out = []
    # the structured blocks, one of each shape (block 5 with the exotic run) per switch set of the test
    for extra in tb.STRUCTURED_EXTRAS:
        def structured(it, extra=extra):
            rng = np.random.default_rng(1234 + len(extra))
            for i in range(it + 1):
                d = tb._structured_block(rng, i)[0]
                rng.choice([1, 2, 8, 256])              # (the test draws the block's starting points here)
            return d
        for it in (1, 2, 3, 4, 5, 6):
            out.append(("structured_%d" % it, ",".join(x for x in (SMALL, extra) if x), None, lambda it=it, f=structured: f(it), (1, 2, 8, 256)[it % 4]))
    out.append(("deep_repeats", "", None, lambda: tb._deep_repeat_block(4 << 20), 8))
    for shape in ("", "BWTC_HIP_FIN_WINDOW=2048,BWTC_HIP_FIN_GROUP=1024"):
        for i, name in enumerate(("repeated_lines", "four_copies")):
            out.append(("mostly_tied_" + name, shape, None, lambda i=i: tb._mostly_tied_blocks(4 << 20)[i][1], 8))
    for extra in ("", "BWTC_HIP_LONG=0"):
        sw = ",".join(x for x in (SMALL, extra) if x)
        out.append(("run_2pow18", sw, "wide", lambda: tr._long_block(30, "run_2pow18"), 1))
        out.append(("runs_200x300", sw, "wide", lambda: tr._long_block(200, "runs_200x300"), 2))
        out.append(("period_7_stretch", sw, "wide", lambda: tp._long_block(30), 8))
    out.append(("period_3_first_round", "", None, lambda: pc.stretch(3, 1 << 18), 8))
    out.append(("period_257_deferred", "", None, lambda: pc.stretch(257, 1 << 18), 8))
    out.append(("random_bytes", "", "32", lambda: np.random.default_rng(3).integers(0, 256, 300000).astype(np.uint8), 8))
    out.append(("four_letters", "", "32", lambda: synth.gen_dna(1 << 20, 2), 8))
    blocks = {}
    for i, row in enumerate(switch_rows()):
        def one(i=i):
            if not blocks:
                blocks["all"] = tb._switch_blocks(4 << 20)
            return blocks["all"][i % 3]
        out.append(("switch_row_%s" % ("text", "zeros", "repeats")[i % 3], row, None, one, 7))
    return out + step_cases()


def step_cases():
    """The blocks of the closed-form steps (tests/mixedcases.py, periodcases.py), each with BWTC_HIP_MIXED=1 and without."""
    def noise_with_stretch():
        d = np.random.default_rng(9).integers(0, 256, 200000).astype(np.uint8)
        d[50000:50400] = pc.stretch(257, 400)
        return d
    one = []
    for p, name in ((9, "merged"), (300, "deferred")):
        for sp in (1, 8):
            one.append(("run_and_stretch_%d_%s" % (p, name), "", None, lambda p=p: mc.run_and_stretch(p, 1 << 16, 1 << 16), sp))
    one.append(("short_runs_beside_stretches", "", None, lambda: mc.short_runs_beside_stretches(64, 16), 8))
    for i, name in ((0, "run_into_stretch_falling"), (3, "stretch_into_run_rising")):
        one.append(("seam_" + name, "", None, lambda i=i: mc.seam_blocks(9)[i][1], 8))
    for i, name in enumerate(("zeros", "one_run_in_noise", "one_stretch_without_runs", "random_bytes", "generator_text")):
        one.append(("plain_" + name, "", None, lambda i=i: mc.plain_blocks()[i][1], 8))
    for extra in ("", ",BWTC_HIP_FINISHER=0", ",BWTC_HIP_PERIOD=64", ",BWTC_HIP_PERIOD=128", ",BWTC_HIP_PERIOD=66", ",BWTC_HIP_PERIOD=1"):
        one.append(("run_and_stretch_64", SMALL + extra, "wide", lambda: mc.run_and_stretch(64, 1 << 16, 1 << 16), 8))
    # a waiting step whose gate closes at depth 512 before it runs (forced: the worth test does not remove it first)
    one.append(("stretch_257x400_in_noise", "BWTC_HIP_PERIOD=257", None, noise_with_stretch, 8))
    for sw in ("BWTC_HIP_RUNS=0", "BWTC_HIP_PERIODS=0"):          # (RUNS=0: the trial pass of period 1)
        one.append(("period_3_first_round", sw, None, lambda: pc.stretch(3, 1 << 18), 8))
        one.append(("period_257_deferred", sw, None, lambda: pc.stretch(257, 1 << 18), 8))
    out = []
    for name, sw, plan, make, sp in one:
        out.append((name, sw, plan, make, sp))
        out.append((name, ",".join(x for x in (sw, MIXED) if x), plan, make, sp))
    return out


def said_by(call):
    """call()'s result and the sorter's debug output of it (as scripts/mixed_bench.py's debug_lines)."""
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["BWTC_HIP_DEBUG"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            got = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["BWTC_HIP_DEBUG"]
        tmp.seek(0)
        return got, tmp.read().decode("utf-8", "replace")


def step_sights(sw, steps, said):
    """Which of STEP_SIGHTS a block of a context with the switch shows."""
    run_depth, _, period_depth = steps[:3]
    seen = set()
    if run_depth == period_depth > 0:
        seen.add(STEP_SIGHTS[0])
    if 0 < run_depth < period_depth:
        seen.add(STEP_SIGHTS[1])
    ran = [i for i, x in enumerate(said) if x.startswith("runs:") and x.endswith(": run step")]
    if ran and any(x.endswith("no period step") for x in said[ran[0]:]):
        seen.add(STEP_SIGHTS[2])
    forced = [x for x in sw.split(",") if x.startswith("BWTC_HIP_PERIOD=")]
    if forced and forced[0] != "BWTC_HIP_PERIOD=1" and period_depth == 0:
        seen.add(STEP_SIGHTS[3])
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sink = open(args.out, "w") if args.out else sys.stdout
    by_switch = {}
    for c in cases():
        by_switch.setdefault(c[1], []).append(c)
    touched = set(x.split("=")[0] for sw in by_switch for x in sw.split(",") if x)
    union, clear, sights = 0, set(), set()
    for sw, group in by_switch.items():
        for name in touched:
            os.environ.pop(name, None)
        for one in sw.split(","):
            if one:
                name, value = one.split("=")
                os.environ[name] = value
        built = [(c, np.ascontiguousarray(c[3](), dtype=np.uint8)) for c in group]
        assert all(d.size <= 4 << 20 for _, d in built)
        with hip.Context(0, max(d.size for _, d in built)) as ctx:
            for (name, _, plan, _, sp), d in built:
                (bwt, lf, _), said = said_by(lambda: ctx.bwt_block(d, sp))
                said = [TOOK.sub("took * ms", x) for x in said.splitlines() if x.startswith(SAID)]
                st = ctx.stats()
                union |= st.route
                if not st.route & 1 and plan:
                    clear.add(plan)
                line = {"case": name, "switches": sw, "bytes": int(d.size), "starting_points": sp,
                        "sha256": hashlib.sha256(bwt.tobytes()).hexdigest(), "lf": [int(x) for x in lf], "pidx": int(lf[0]),
                        "rounds": st.rounds, "route": st.route, "active_sum": st.active_sum, "sort_pass_items": st.sort_pass_items,
                        "finisher_entries": st.finisher_entries, "alg_bytes": st.alg_bytes, "period_get": list(ctx.period()),
                        "steps_get": list(ctx.steps()), "said": said}
                if name in VOTES_VARY:
                    line["period_get"][2] = None
                    line["said"] = [VOTES.sub("with * votes", x) for x in said]
                if MIXED in sw.split(","):
                    sights |= step_sights(sw, line["steps_get"], said)
                sink.write(json.dumps(line) + "\n")
                sink.flush()
    missing = [b for b in WANT_BITS if not union >> b & 1]
    assert not missing, "route bits never set: %s (union %#x)" % (missing, union)
    assert clear == {"wide", "32"}, "no block without the long keys on the key plans %s" % sorted({"wide", "32"} - clear)
    assert sights == set(STEP_SIGHTS), "never seen with %s: %s" % (MIXED, sorted(set(STEP_SIGHTS) - sights))
    print("sorter_trace: %d cases, route bits %#x" % (sum(len(g) for g in by_switch.values()), union), file=sys.stderr)


if __name__ == "__main__":
    main()
