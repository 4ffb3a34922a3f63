#!/usr/bin/env python3
"""What BWTC_HIP_MULTI=1 -- closed-form steps for several periods in one block -- buys and costs, on one GPU: one JSON
line per 256 MiB block.

Blocks: the generator's text with a 64 MiB stretch of period 9 and a 64 MiB stretch of period 12; with three record
widths (24, 40, 100), 48 MiB each; with the period-9 stretch and a period-256 byte ramp (a deferred step); the merge case
-- three equal period-9 stretches and three equal period-12 stretches of 16 MiB behind equal tails; and what the switch
must not slow down -- the plain text, the text with the period-9 stretch alone, all zeros, and BWTC_HIP_MIXED's block
with a zero run and the period-9 stretch.  Every block is transformed on the device by three contexts -- with
BWTC_HIP_MULTI=1, with BWTC_HIP_MIXED=1 and with neither -- --reps times each in rotating order, and every result is
taken back through the GPU inverse and compared with the block.

Every block is measured by a child process of its own under a time limit (--limit seconds): a block that goes silent
costs its limit and its line, not the session.

A line holds, for "multi", "mixed" and "off": ms_total and ms_sort of every repeat and their smallest, rounds,
active_sum, route, alg_bytes and sort_pass_items; Context.schedule() with the switch; and, from one extra transform per
context with the sorter's debug lines, the vote kernel's, the period-length passes' and the trial passes' own times.

--parent DIR: a tree of the commit before the feature, built (DIR/bwtc_amd with its library).  The plain-text control is
then measured once more by a child that imports that tree, and its line (block "control_text", build "parent") holds the
numbers that must not move: rounds, route, alg_bytes, sort_pass_items, and the times.

Usage: scripts/multi_bench.py [--mib 256] [--reps 3] [--only NAME[,NAME]] [--tag TEXT] [--out FILE] [--limit 240] [--parent DIR]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("BWTC_BENCH_ROOT") or HERE          # (the tree whose bwtc_amd is measured: --parent sets it for one child)
sys.path.insert(0, ROOT)

PASS_LINE = re.compile(r"periods: the period-length pass took ([0-9.]+) ms")
TRIAL_LINE = re.compile(r"periods: a trial pass \(no lengths stored\) took ([0-9.]+) ms")
RUN_PASS_LINE = re.compile(r"runs: the run-length pass took ([0-9.]+) ms")
VOTE_LINE = re.compile(r"periods: the vote kernel took ([0-9.]+) ms for (\d+) entries")
STEPS_LINE = re.compile(r"steps: .*")

NAMES = ["text_periods_9_12", "text_records_24_40_100", "text_period_9_and_256_ramp", "merge_case_9_12",
         "control_text", "control_text_period_9", "control_zeros", "control_text_run_and_period_9"]
MODES = {"multi": "BWTC_HIP_MULTI", "mixed": "BWTC_HIP_MIXED", "off": None}


def make(name, size):
    import numpy as np
    from bwtc_amd import synth

    def tiled(unit, n):
        return np.tile(unit, n // unit.size + 1)[:n].copy()

    def put(d, at, unit, n):
        d[at:at + n] = tiled(unit, n)

    abc9, abc12 = np.frombuffer(b"abcabcabd", np.uint8), np.frombuffer(b"abcdabcdabce", np.uint8)
    if name == "control_zeros":
        return np.zeros(size, np.uint8)
    d = synth.gen_text(size, 3).copy()
    if name == "control_text":
        return d
    if name == "control_text_period_9":
        put(d, size // 2, abc9, size // 4)
    elif name == "control_text_run_and_period_9":
        d[size // 8:size // 8 + size // 4] = 0
        put(d, size // 2, abc9, size // 4)
    elif name == "text_periods_9_12":
        put(d, size // 8, abc12, size // 4)
        put(d, size // 2, abc9, size // 4)
    elif name == "text_period_9_and_256_ramp":
        put(d, size // 8, np.arange(256, dtype=np.uint8), size // 4)
        put(d, size // 2, abc9, size // 4)
    elif name == "text_records_24_40_100":
        rng = np.random.default_rng(24)
        for i, w in enumerate((24, 40, 100)):
            unit = rng.integers(32, 127, w).astype(np.uint8)
            unit[-1] = 10                                  # (a record ends in a newline, and nowhere else)
            put(d, (1 + 5 * i) * (size // 16), unit, 3 * (size // 16))
    elif name == "merge_case_9_12":
        tail = d[:48].copy()
        for i in range(6):                                 # (the sorter sees the block reversed: the equal bytes go before a stretch here)
            at = (1 + 2 * i) * (size // 16)
            put(d, at, abc9 if i < 3 else abc12, size // 16)
            d[at - 48:at] = tail
    else:
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
    for switch in MODES.values():
        if switch:
            os.environ.pop(switch, None)
    if MODES[mode]:
        os.environ[MODES[mode]] = "1"
    ctx = hip.Context(0, size)
    if MODES[mode]:
        del os.environ[MODES[mode]]
    return ctx


def child(name, args):
    """One block, measured in this process; the JSON line on stdout."""
    size = args.mib << 20
    modes = [m for m in args.modes.split(",") if m]
    ctxs = {m: context(m, size) for m in modes}
    first = ctxs[modes[0]]
    d_in, d_out, d_back = (first.dmalloc(size + 64) for _ in range(3))
    data = make(name, size)
    line = {"block": name, "block_bytes": size, "reps": args.reps}
    if args.tag:
        line["build"] = args.tag
    runs = {m: [] for m in modes}
    first.to_device(d_in, data)                               # (the transform leaves its input as it is)
    for rep in range(args.reps):
        for m in modes[rep % len(modes):] + modes[:rep % len(modes)]:
            ctx = ctxs[m]
            lf, _ = ctx.bwt_block_device(d_in, d_out, size, 8)
            st = ctx.stats()
            runs[m].append({"ms_total": round(st.ms_total, 3), "ms_sort": round(st.ms_sort, 3), "rounds": st.rounds, "active_sum": st.active_sum,
                            "route": st.route, "alg_bytes": st.alg_bytes, "sort_pass_items": st.sort_pass_items})
            ctx.inverse_bwt_block_device(d_out, d_back, size, lf)
            assert (ctx.to_host(d_back, size) == data).all(), (name, m, rep)
    for m, rr in runs.items():
        assert len({(r["rounds"], r["active_sum"], r["route"], r["alg_bytes"], r["sort_pass_items"]) for r in rr}) == 1, rr   # the block's, not the repeat's
        line[m] = {"ms_total": min(r["ms_total"] for r in rr), "ms_sort": min(r["ms_sort"] for r in rr),
                   "ms_total_all": [r["ms_total"] for r in rr], "ms_sort_all": [r["ms_sort"] for r in rr]}
        line[m].update({k: rr[0][k] for k in ("rounds", "active_sum", "route", "alg_bytes", "sort_pass_items")})
    for m, ctx in ctxs.items():
        said = debug_lines(lambda: ctx.bwt_block_device(d_in, d_out, size, 8))
        v = VOTE_LINE.search(said)
        line[m].update(vote_kernel_ms=float(v.group(1)) if v else None, vote_kernel_entries=int(v.group(2)) if v else None,
                       run_length_pass_ms=[float(x) for x in RUN_PASS_LINE.findall(said)],
                       period_length_pass_ms=[float(x) for x in PASS_LINE.findall(said)],
                       trial_pass_ms=[float(x) for x in TRIAL_LINE.findall(said)])
        if m != "off":
            s = STEPS_LINE.search(said)
            line[m]["said"] = s.group(0) if s else None
        if hasattr(ctx, "schedule"):
            line[m]["schedule"] = ctx.schedule()
    for q in (d_in, d_out, d_back):
        first.dfree(q)
    for ctx in ctxs.values():
        ctx.close()
    print("LINE " + json.dumps(line), flush=True)


def measure(name, args, modes, tag, root=None):
    """One child under the time limit -> its line, or None."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--mib", str(args.mib), "--reps", str(args.reps), "--tag", tag, "--modes", modes]
    env = dict(os.environ)
    if root:
        env["BWTC_BENCH_ROOT"] = os.path.abspath(root)
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit, env=env)
    except subprocess.TimeoutExpired:
        print("%s: no line within %d s; stopping here" % (name, args.limit), flush=True)
        return None                                           # (nothing more on a GPU that may be busy with what was cut short)
    if done.returncode != 0:
        print("%s: the child ended with status %d; stopping here" % (name, done.returncode), flush=True)
        return None
    lines = [x[5:] for x in done.stdout.decode().splitlines() if x.startswith("LINE ")]
    assert len(lines) == 1, done.stdout[-2000:]
    print(lines[0], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:                            # (line by line: a run cut short keeps what it measured)
        f.write(lines[0] + "\n")
    return lines[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "multi_steps_bench.jsonl"))
    ap.add_argument("--parent", default="", help="a built tree of the commit before the feature: the plain-text control on it too")
    ap.add_argument("--child", default="")
    ap.add_argument("--modes", default="multi,mixed,off")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    only = [x for x in args.only.split(",") if x]
    for name in NAMES:
        if only and name not in only:
            continue
        if measure(name, args, "multi,mixed,off", args.tag) is None:
            return 1
        if name == "control_text" and args.parent:
            if measure(name, args, "off", "parent", args.parent) is None:
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
