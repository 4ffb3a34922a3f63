#!/usr/bin/env python3
"""What the suffix sorter does with a fixed list of small blocks, on one GPU: one JSON line per case, no times.

A line holds the case's name and switch set, the block's size and starting points, SHA-256 of the transformed bytes, the
LF powers, pidx (LF[0]), stats.rounds / route / active_sum / sort_pass_items / finisher_entries / alg_bytes, what
bwtc_hip_period_get, bwtc_hip_steps_get, bwtc_hip_schedule_get and bwtc_hip_copies_get say, and the sorter's debug lines
that begin with "runs:", "periods:", "steps:", "copies:", "finisher:", "finisher pass", "local pass:" or "shallow groups:",
their measured times masked ("took * ms"):
every stretch-length pass (storing or trial, with its period), the vote kernel and each decision, and every finisher
pass and local step with its counts and depths.  Two builds of the library whose traces are equal line for line sorted these blocks by
the same routes, with the same passes in the same order and the same launch-independent counters, to the same bytes:
the check of a change to the sorter's host code that is meant to change nothing.

The blocks come from the tests' own builders (tests/test_gpu_bwt.py, test_gpu_run_ranks.py, test_gpu_period_step.py,
periodcases.py, mixedcases.py, multicases.py, longcases.py, copycases.py), at 4 MiB at most.  A switch is read when a
context is made: every switch set gets a context of its own, one at a time.  The tool itself asserts that the cases
between them set every route bit it names in WANT_BITS, that a block without the long keys (route bit 0 clear) was seen
on a 64-bit key plan and on the 32-bit one, that the cases with BWTC_HIP_MIXED=1 showed every way the two closed-form
steps meet in one block (STEP_SIGHTS), and that those with BWTC_HIP_MULTI=1 and BWTC_HIP_LONG_PERIODS=1 showed
MULTI_SIGHTS and LONG_SIGHTS -- equal traces over cases that all took one route would say little.  The last of
LONG_SIGHTS, a long winner that the division reduced, is shown by none of the cases: the tool ends with that assertion
failing (exit status 1) behind a complete trace; see the comment at LONG_SIGHTS.

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

import copycases as cc                    # noqa: E402
import longcases as lc                    # noqa: E402
import mixedcases as mc                   # noqa: E402
import multicases as mu                   # noqa: E402
import periodcases as pc                  # noqa: E402
import test_gpu_bwt as tb                 # noqa: E402
import test_gpu_copy_rounds as tc         # noqa: E402
import test_gpu_period_step as tp         # noqa: E402
import test_gpu_run_ranks as tr           # noqa: E402
from bwtc_amd import hip, synth           # noqa: E402

SMALL = "BWTC_HIP_GRAM_MIN_N=64"          # as the tests do: small blocks through the gram / long-key routes (and a 64-bit key plan)
# Route bit 7 (a finisher pass's lists would not fit) is not wanted: it takes a list of more than 8 Mi entries in a
# context made for exactly the block (m / 64 > cap / 128 + 65536), which no block of 4 MiB has.
# test_wide_finisher_shape_on_blocks_that_are_mostly_tied covers it at 16 MiB.
WANT_BITS = (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11)
# The vote count of bwtc_hip_period_get is printed as null for these: the finder counts neighbours of one group in a
# list whose order inside a group the finisher's atomic appends decide, and on the block with the planted run of three
# rare symbols one build's count differs from run to run by a few votes in 2900 (threshold: 256).  Nothing else does.
VOTES_VARY = ("structured_5",)
MIXED = "BWTC_HIP_MIXED=1"
MULTI, COPIES, LONG = "BWTC_HIP_MULTI=1", "BWTC_HIP_COPIES=1", "BWTC_HIP_LONG_PERIODS=1"
# What the cases with the switch must show between them (main's closing assertion)
STEP_SIGHTS = ("one period step that ranked the runs too", "a period step behind the run step", "no period step after a run step",
               "no period step under a forced period")
# ... and the finisher's own lines: each pass's entries in and out with the hard and shallow counts and depths, what goes on
# to the rounds, the shallow groups' leftovers and the local list's steps, in order
SAID = ("runs:", "periods:", "steps:", "copies:", "finisher:", "finisher pass", "local pass:", "shallow groups:")
# What the cases with BWTC_HIP_MULTI=1 and those with BWTC_HIP_LONG_PERIODS=1 must show between them
MULTI_SIGHTS = ("two or more period entries", "the first period entry ranked the runs too", "a dropped entry", "exactly one accepted period")
# The last of these is NOT MET, by this sorter or by the one before the step record: the closing assertion fails on it,
# behind a complete trace (every line is written before anything is asserted).  None of the cases has a long winner that
# the division reduces -- the sorter's own list is in position order and votes for the period itself, as
# tests/test_gpu_long_period_step.py says of its 4 MiB blocks.  What the cases show: long winners 4097, 8192, 4100 and
# 65536 with trial passes of 241 and 17, 4096, 2050 / 820 / 100 and 32768, all in vain; and 352 further transforms --
# multiple_block(4100 / 1025), back_to_back, the generator's text of 5000, 300 and 4100 bytes tiled, stretches of period
# 1025 and 4100, each with and without the switch under ten route switches, 1 and 8 starting points -- reduced no winner,
# short or long.  So no line proves the branch of weigh_period that divides a winner; that branch keeps the handling of
# the lengths it had before the step record.  Over a given list the division is tests/test_gpu_long_period_votes.py's.
LONG_SIGHTS = ("a step with p > 4096", "a long winner whose quotients the division tried", "a long winner that the division reduced")
PASS = re.compile(r"periods: (?:the period-length pass|a trial pass \(no lengths stored\)) took \* ms for [0-9]+ suffixes, period ([0-9]+)")
TOOK = re.compile(r"(took|marks|flags|lengths) [0-9.]+ ms")    # (the three times of a copy pass: "marks * ms, flags * ms, lengths * ms")
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
    return out + step_cases() + multi_cases() + long_cases() + copy_cases()


def multi_cases():
    """The blocks of several periods (tests/multicases.py, as tests/test_gpu_multi_steps.py hands them over) with
    BWTC_HIP_MULTI=1, the one-period blocks that are MIXED's under it, and a forced period under it."""
    def noise_with_stretch():
        d = np.random.default_rng(9).integers(0, 256, 200000).astype(np.uint8)
        d[50000:50400] = pc.stretch(257, 400)
        return d
    out = [("pair_%d_%d" % pair, MULTI, None, lambda pair=pair: mu.block(mu.stretches(pair, 1 << 16)), 8) for pair in (mu.PAIRS[3],)]
    out.append(("divisor_pair", MULTI, None, lambda: mu.block(mu.stretches(mu.DIVISOR_PAIR, 1 << 16)), 8))
    for planted in sorted(mu.TRIPLES):
        out.append(("triple_%d_%d_%d" % planted, MULTI, None, lambda planted=planted: mu.block(mu.stretches(planted, 1 << 16)), 1))
    out.append(("merge_case", MULTI, None, lambda: mu.block(mu.merge_case()), 8))
    out.append(("seam_9_12_into_each_other", MULTI, None, lambda: mu.block(mu.seam_blocks(9, 12)[0][1]), 8))
    for it in (0, 1):
        out.append(("multi_random_%d" % it, MULTI, None, lambda it=it: mu.block(mu.random_block(it)[0]), (1, 8)[it % 2]))
    out.append(("pair_9_300_and_a_run", MULTI, None, lambda: mu.block(mu.stretches((9, 300), 1 << 16, run=1 << 16)), 8))
    # one accepted period or none: MIXED's schedule
    for p in (9, 300):
        out.append(("run_and_stretch_%d" % p, MULTI, None, lambda p=p: mc.run_and_stretch(p, 1 << 16, 1 << 16), 8))
    out.append(("one_stretch_of_period_9", MULTI, None, lambda: mu.block(mu.stretches((9,), 1 << 16)), 8))
    out.append(("plain_random_bytes", MULTI, None, lambda: mc.plain_blocks()[3][1], 8))
    # a forced period under the switch: one candidate, no votes; the waiting step's gate closes at depth 512 (flag 2)
    out.append(("stretch_257x400_in_noise", MULTI + ",BWTC_HIP_PERIOD=257", None, noise_with_stretch, 8))
    out.append(("pair_9_300", MULTI + ",BWTC_HIP_PERIOD=9", None, lambda: mu.block(mu.stretches((9, 300), 1 << 16)), 8))
    return out


def long_cases():
    """The blocks of the periods above 4096 (tests/longcases.py, as tests/test_gpu_long_period_step.py hands them over)."""
    out = [("long_one_stretch_4097", LONG, None, lambda: lc.one_stretch(4097), 8),
           ("long_one_stretch_8192_text", LONG, None, lambda: lc.one_stretch(8192, "text"), 1),
           ("long_worth_4097_below", LONG, None, lambda: lc.worth_block(4097, -1), 8),
           ("long_worth_4097_at", LONG, None, lambda: lc.worth_block(4097, 0), 8),
           ("long_division_4100", LONG, None, lambda: lc.division_block(4100), 8),
           ("long_back_to_back", LONG, None, lc.back_to_back, 8),
           ("long_forced_4999", LONG + ",BWTC_HIP_LONG_PERIOD=4999", None, lambda: lc.forced_block(4999), 8),
           ("long_and_short", LONG + "," + MULTI, None, lc.long_and_short, 8),
           ("long_back_to_back", LONG + "," + COPIES, None, lc.back_to_back, 8)]
    return out


def copy_cases():
    """The copy blocks of tests/test_gpu_copy_rounds.py and one block without copies, with BWTC_HIP_COPIES=1."""
    out = [("copies_%d" % i, COPIES, None, lambda i=i: cc.block(tc._copy_blocks()[i][1]), (1, 8)[i % 2]) for i in range(len(tc._copy_blocks()))]
    out.append(("copies_none_random_bytes", COPIES, None, lambda: cc.block(cc.plain_blocks()[0][1]), 8))
    return out


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


def multi_sights(schedule, said):
    """Which of MULTI_SIGHTS a block of a context with BWTC_HIP_MULTI=1 shows.  A block whose steps merge (two or three
    accepted periods) says "steps: N entries"; one accepted period leaves MIXED's schedule and MIXED's line."""
    periods = [e for e in schedule if e[0] >= 2]
    seen = set()
    if len(periods) >= 2:
        seen.add(MULTI_SIGHTS[0])
    if periods and periods[0][4] & 1:
        seen.add(MULTI_SIGHTS[1])
    if any(e[4] & 2 for e in schedule):
        seen.add(MULTI_SIGHTS[2])
    if len(periods) == 1 and not any(re.match(r"steps: [0-9]+ entries", x) for x in said):
        seen.add(MULTI_SIGHTS[3])
    return seen


def long_sights(schedule, period, said):
    """Which of LONG_SIGHTS a block of a context with BWTC_HIP_LONG_PERIODS=1 shows.  The division: the winner's pass, the
    trial passes of its quotients, and -- where one was kept -- a last pass of the period that is left, a proper divisor."""
    seen = set()
    if any(e[0] > 4096 and e[1] for e in schedule):
        seen.add(LONG_SIGHTS[0])
    passes = [int(p) for x in said for p in PASS.findall(x)]
    trials = [int(p) for x in said if "a trial pass" in x for p in PASS.findall(x)]
    if passes and passes[0] > 4096 and trials and all(passes[0] % q == 0 for q in trials):
        seen.add(LONG_SIGHTS[1])
    if passes and passes[0] > 4096 and 2 <= period[0] < passes[0] and passes[0] % period[0] == 0 and passes[-1] == period[0]:
        seen.add(LONG_SIGHTS[2])
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
                said = [TOOK.sub(r"\1 * ms", x) for x in said.splitlines() if x.startswith(SAID)]
                st = ctx.stats()
                union |= st.route
                if not st.route & 1 and plan:
                    clear.add(plan)
                line = {"case": name, "switches": sw, "bytes": int(d.size), "starting_points": sp,
                        "sha256": hashlib.sha256(bwt.tobytes()).hexdigest(), "lf": [int(x) for x in lf], "pidx": int(lf[0]),
                        "rounds": st.rounds, "route": st.route, "active_sum": st.active_sum, "sort_pass_items": st.sort_pass_items,
                        "finisher_entries": st.finisher_entries, "alg_bytes": st.alg_bytes, "period_get": list(ctx.period()),
                        "steps_get": list(ctx.steps()), "schedule_get": [list(e) for e in ctx.schedule()], "copies_get": list(ctx.copies()),
                        "said": said}
                if MIXED in sw.split(","):
                    sights |= step_sights(sw, line["steps_get"], said)
                if MULTI in sw.split(","):
                    sights |= multi_sights(line["schedule_get"], said)
                if LONG in sw.split(","):
                    sights |= long_sights(line["schedule_get"], line["period_get"], said)
                if name in VOTES_VARY:
                    line["period_get"][2] = None
                    line["said"] = [VOTES.sub("with * votes", x) for x in said]
                sink.write(json.dumps(line) + "\n")
                sink.flush()
    missing = [b for b in WANT_BITS if not union >> b & 1]
    assert not missing, "route bits never set: %s (union %#x)" % (missing, union)
    assert clear == {"wide", "32"}, "no block without the long keys on the key plans %s" % sorted({"wide", "32"} - clear)
    wanted = set(STEP_SIGHTS + MULTI_SIGHTS + LONG_SIGHTS)
    print("sorter_trace: %d cases, route bits %#x" % (sum(len(g) for g in by_switch.values()), union), file=sys.stderr)
    assert sights == wanted, "never seen with %s, %s or %s: %s" % (MIXED, MULTI, LONG, sorted(wanted - sights))


if __name__ == "__main__":
    main()
