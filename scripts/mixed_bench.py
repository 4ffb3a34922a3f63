#!/usr/bin/env python3
"""What BWTC_HIP_MIXED=1 -- the run step AND a period step in one block -- buys and costs, on one GPU: one JSON line per
256 MiB block.

Blocks: the generator's text with a 64 MiB zero run and a 64 MiB stretch of period 9 (abcabcabd); the same with a
stretch of period 256 (a byte ramp: a deferred step); and what the switch must not slow down -- all zeros, the text
with the zero run alone, the plain text.  Every block is transformed on the device by two contexts, one with
BWTC_HIP_MIXED=1 and one without, --reps times each in alternating order, and every result is taken back through the
GPU inverse and compared with the block.

Every block is measured by a child process of its own under a time limit (--limit seconds): a block that goes silent
costs its limit and its line, not the session.

A line holds, for "on" and "off": ms_total and ms_sort of every repeat and their smallest, rounds, active_sum and
route; what bwtc_hip_steps_get and bwtc_hip_period_get say with the switch; and, from one extra transform per context
with the sorter's debug lines, the vote kernel's, the period-length passes' and the trial passes' own times -- what
the switch adds to a block that has nothing mixed.

--passes: instead of blocks, the stretch-length pass alone through its test hooks, for periods 9 and 256 over
--mib MiB of text with a run and a stretch: the pass's own time (the sorter's debug line) without and with the second
maximum, --reps times each in alternating order.

Usage: scripts/mixed_bench.py [--mib 256] [--reps 5] [--only NAME[,NAME]] [--tag TEXT] [--out FILE] [--limit 240] [--passes]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PASS_LINE = re.compile(r"periods: the period-length pass took ([0-9.]+) ms")
TRIAL_LINE = re.compile(r"periods: a trial pass \(no lengths stored\) took ([0-9.]+) ms")
RUN_PASS_LINE = re.compile(r"runs: the run-length pass took ([0-9.]+) ms")
VOTE_LINE = re.compile(r"periods: the vote kernel took ([0-9.]+) ms for (\d+) entries")
STEPS_LINE = re.compile(r"steps: .*")

NAMES = ["text_run_and_period_9", "text_run_and_period_256_ramp", "control_zeros", "control_text_run", "control_text"]


def make(name, size):
    import numpy as np
    from bwtc_amd import synth

    def tiled(unit, n):
        return np.tile(unit, n // unit.size + 1)[:n].copy()

    if name == "control_zeros":
        return np.zeros(size, np.uint8)
    d = synth.gen_text(size, 3).copy()
    if name == "control_text":
        return d
    d[size // 8:size // 8 + size // 4] = 0
    if name == "text_run_and_period_9":
        d[size // 2:size // 2 + size // 4] = tiled(np.frombuffer(b"abcabcabd", np.uint8), size // 4)
    elif name == "text_run_and_period_256_ramp":
        d[size // 2:size // 2 + size // 4] = tiled(np.arange(256, dtype=np.uint8), size // 4)
    elif name != "control_text_run":
        raise SystemExit("unknown block " + name)
    return d


def debug_lines(call):
    """The sorter's debug output of one call."""
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["BWTC_HIP_DEBUG"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["BWTC_HIP_DEBUG"]
        tmp.seek(0)
        return tmp.read().decode("utf-8", "replace")


def context(mode, size):
    from bwtc_amd import hip
    os.environ.pop("BWTC_HIP_MIXED", None)
    if mode == "on":
        os.environ["BWTC_HIP_MIXED"] = "1"
    ctx = hip.Context(0, size)
    os.environ.pop("BWTC_HIP_MIXED", None)
    return ctx


def child(name, args):
    """One block, measured in this process; the JSON line on stdout."""
    size = args.mib << 20
    ctx_on, ctx_off = context("on", size), context("off", size)
    d_in, d_out, d_back = (ctx_on.dmalloc(size + 64) for _ in range(3))
    data = make(name, size)
    line = {"block": name, "block_bytes": size, "reps": args.reps}
    if args.tag:
        line["build"] = args.tag
    runs = {"on": [], "off": []}
    ctx_on.to_device(d_in, data)                              # (the transform leaves its input as it is)
    for rep in range(args.reps):
        for mode, ctx in (("on", ctx_on), ("off", ctx_off)) if rep % 2 == 0 else (("off", ctx_off), ("on", ctx_on)):
            lf, _ = ctx.bwt_block_device(d_in, d_out, size, 8)
            st = ctx.stats()
            runs[mode].append({"ms_total": round(st.ms_total, 3), "ms_sort": round(st.ms_sort, 3), "rounds": st.rounds,
                               "active_sum": st.active_sum, "route": st.route})
            ctx.inverse_bwt_block_device(d_out, d_back, size, lf)
            assert (ctx.to_host(d_back, size) == data).all(), (name, mode, rep)
    for mode, rr in runs.items():
        assert len({(r["rounds"], r["active_sum"], r["route"]) for r in rr}) == 1, rr       # the route is the block's, not the repeat's
        line[mode] = {"ms_total": min(r["ms_total"] for r in rr), "ms_sort": min(r["ms_sort"] for r in rr),
                      "ms_total_all": [r["ms_total"] for r in rr], "ms_sort_all": [r["ms_sort"] for r in rr],
                      "rounds": rr[0]["rounds"], "active_sum": rr[0]["active_sum"], "route": rr[0]["route"],
                      "GBps": round(size / (min(r["ms_total"] for r in rr) * 1e-3) / 1e9, 2)}
    for mode, ctx in (("on", ctx_on), ("off", ctx_off)):
        said = debug_lines(lambda: ctx.bwt_block_device(d_in, d_out, size, 8))
        m = VOTE_LINE.search(said)
        line[mode].update(vote_kernel_ms=float(m.group(1)) if m else None, vote_kernel_entries=int(m.group(2)) if m else None,
                          run_length_pass_ms=[float(x) for x in RUN_PASS_LINE.findall(said)],
                          period_length_pass_ms=[float(x) for x in PASS_LINE.findall(said)],
                          trial_pass_ms=[float(x) for x in TRIAL_LINE.findall(said)])
        if mode == "on":
            m = STEPS_LINE.search(said)
            line["said"] = m.group(0) if m else None
    line["steps_get"] = dict(zip(("run_depth", "period_p", "period_depth", "longest_run", "longest_proper"), ctx_on.steps()))
    line["period_get"] = dict(zip(("p", "longest", "votes", "step_depth"), ctx_on.period()))
    for q in (d_in, d_out, d_back):
        ctx_on.dfree(q)
    ctx_on.close()
    ctx_off.close()
    print("LINE " + json.dumps(line), flush=True)


def passes(args):
    """The stretch-length pass through its hooks, without and with the second maximum."""
    import numpy as np
    from bwtc_amd import hip
    size = args.mib << 20
    data = make("text_run_and_period_9", size)
    k_out = np.zeros(size, np.uint32)
    line = {"block": "stretch_length_pass", "block_bytes": size, "reps": args.reps}
    if args.tag:
        line["build"] = args.tag
    with hip.Context(0, size) as ctx:
        for p in (9, 256):
            took = {"plain": [], "proper": []}
            for rep in range(args.reps + 1):                  # (the first repeat of each is the warm-up)
                for mode in ("plain", "proper") if rep % 2 == 0 else ("proper", "plain"):
                    hook = ctx.test_period_lengths if mode == "plain" else ctx.test_period_proper
                    said = debug_lines(lambda: hook(data, p, k_out))
                    if rep:
                        took[mode].append(float(PASS_LINE.search(said).group(1)))
            line["p_%d" % p] = {"plain_ms": took["plain"], "proper_ms": took["proper"], "plain_min": min(took["plain"]), "proper_min": min(took["proper"])}
    print("LINE " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_steps_bench.jsonl"))
    ap.add_argument("--child", default="")
    ap.add_argument("--passes", action="store_true", help="the stretch-length pass alone, without and with the second maximum")
    args = ap.parse_args()
    if args.child == "stretch_length_pass":
        return passes(args)
    if args.child:
        return child(args.child, args)
    only = [x for x in args.only.split(",") if x]
    for name in ["stretch_length_pass"] if args.passes else NAMES:
        if only and name not in only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--mib", str(args.mib), "--reps", str(args.reps), "--tag", args.tag]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("%s: no line within %d s; stopping here" % (name, args.limit), flush=True)
            return 1                                          # (nothing more on a GPU that may be busy with what was cut short)
        if done.returncode != 0:
            print("%s: the child ended with status %d; stopping here" % (name, done.returncode), flush=True)
            return 1
        lines = [x[5:] for x in done.stdout.decode().splitlines() if x.startswith("LINE ")]
        assert len(lines) == 1, done.stdout[-2000:]
        print(lines[0], flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:                        # (line by line: a run cut short keeps what it measured)
            f.write(lines[0] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
