#!/usr/bin/env python3
"""What the suffix sorter's period step buys, on one GPU: one JSON line per 256 MiB block.

Blocks of one period (9: abcabcabd; 2; 256: a byte ramp; 4096 random bytes), the generator's text with one 64 MiB
stretch of period 9, fixed-width records (a 64-byte unit with 8 random bytes per record: no exact period) and controls
(all zeros: the run step; the generator's plain text; `realtext`, bench.py's workload, as shipped -- it takes the run
step and so never looks for a period -- and with BWTC_HIP_RUNS=0 in both contexts: a long list that pays the votes and
nothing else).  Every block is transformed on the device by two contexts, one as shipped and one with
BWTC_HIP_PERIODS=0, --reps times each in alternating order, and every result is taken back through the GPU inverse and
compared with the block.

Every block is measured by a child process of its own under a time limit (--limit seconds): a block that goes silent
costs its limit and its line, not the session.  The slowest block to check comes last.

A line holds, for "on" and "off": ms_total and ms_sort of every repeat and their smallest, rounds, active_sum and
route; what bwtc_hip_period_get says; the vote kernel's, the period-length pass's and the trial passes' own times
(the sorter's debug lines, from one extra transform), the pass's traffic of 8 bytes per byte over its time and
bwtc_hip_copy_probe beside it.

Usage: scripts/periods_bench.py [--mib 256] [--reps 5] [--only NAME[,NAME]] [--tag TEXT] [--out FILE] [--limit 240] [--off-first]
(BWTC_HIP_LIB=<another build's libbwtc_hip.so> measures that build: --tag names it in the lines.)"""
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
VOTE_LINE = re.compile(r"periods: the vote kernel took ([0-9.]+) ms for (\d+) entries")
SAID_LINE = re.compile(r"periods: period .*")

NAMES = ["period_9", "period_2", "period_256_ramp", "period_4096_random", "text_one_quarter_period_9", "records_64_with_8_random",
         "control_zeros", "control_text", "control_realtext_runs_off", "control_realtext"]        # (last: the longest list, the slowest to make and to check)


def make(name, size):
    import numpy as np
    from bwtc_amd import synth
    rng = np.random.default_rng(5)

    def tiled(unit):
        return np.tile(unit, size // unit.size + 1)[:size].copy()

    if name == "period_9":
        return tiled(np.frombuffer(b"abcabcabd", np.uint8))
    if name == "period_2":
        return tiled(np.frombuffer(b"ab", np.uint8))
    if name == "period_256_ramp":
        return tiled(np.arange(256, dtype=np.uint8))
    if name == "period_4096_random":
        return tiled(rng.integers(0, 256, 4096).astype(np.uint8))
    if name == "text_one_quarter_period_9":
        d = synth.gen_text(size, 3).copy()
        d[size // 4:size // 2] = tiled(np.frombuffer(b"abcabcabd", np.uint8))[:size // 4]
        return d
    if name == "records_64_with_8_random":
        d = tiled(rng.integers(0, 256, 64).astype(np.uint8)).reshape(-1)
        rec = d[:size // 64 * 64].reshape(-1, 64)
        rec[:, 20:28] = rng.integers(0, 256, (rec.shape[0], 8)).astype(np.uint8)
        return d
    if name == "control_zeros":
        return np.zeros(size, np.uint8)
    if name == "control_text":
        return synth.gen_text(size, 3)
    if name in ("control_realtext", "control_realtext_runs_off"):
        sys.path.insert(0, os.path.join(ROOT, "scripts", "r5"))
        import workloads
        return workloads.gen("realtext", size)[0]
    raise SystemExit("unknown block " + name)


def debug_lines(ctx, d_in, d_out, size):
    """The sorter's debug output of one transform."""
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["BWTC_HIP_DEBUG"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            ctx.bwt_block_device(d_in, d_out, size, 8)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["BWTC_HIP_DEBUG"]
        tmp.seek(0)
        return tmp.read().decode("utf-8", "replace")


def child(name, args):
    """One block, measured in this process; the JSON line on stdout."""
    from bwtc_amd import hip
    size = args.mib << 20
    if name.endswith("_runs_off"):
        # (realtext holds runs of blanks above its rounds' first depth: as shipped it takes the run step and never reaches
        # the finder.  With BWTC_HIP_RUNS=0 in both contexts it is the long list that pays the votes and nothing else)
        os.environ["BWTC_HIP_RUNS"] = "0"

    def context(mode):
        os.environ.pop("BWTC_HIP_PERIODS", None)
        if mode == "off":
            os.environ["BWTC_HIP_PERIODS"] = "0"
        ctx = hip.Context(0, size)
        os.environ.pop("BWTC_HIP_PERIODS", None)
        return ctx

    # (the process's second context has measured 0.6 ms per block faster than its first, whatever its switches: --off-first
    # makes the other one first, and the line says which was)
    if args.off_first:
        ctx_off = context("off")
        ctx_on = context("on")
    else:
        ctx_on = context("on")
        ctx_off = context("off")
    probe = ctx_on.copy_probe(1 << 30, 5)
    d_in, d_out, d_back = (ctx_on.dmalloc(size + 64) for _ in range(3))
    data = make(name, size)
    line = {"block": name, "block_bytes": size, "reps": args.reps, "copy_probe_GBps": round(probe, 1),
            "first_context": "off" if args.off_first else "on"}
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
    said = debug_lines(ctx_on, d_in, d_out, size)
    p, longest, votes, depth = ctx_on.period()
    line["period_get"] = {"p": p, "longest": longest, "votes": votes, "step_depth": depth}
    m = SAID_LINE.search(said)
    line["said"] = m.group(0) if m else None
    m = VOTE_LINE.search(said)
    line["vote_kernel_ms"] = float(m.group(1)) if m else None
    line["vote_kernel_entries"] = int(m.group(2)) if m else None
    passes = [float(x) for x in PASS_LINE.findall(said)]
    line["period_length_pass_ms"] = passes
    line["trial_pass_ms"] = [float(x) for x in TRIAL_LINE.findall(said)]
    if passes:
        gbps = 8.0 * size / (min(passes) * 1e-3) / 1e9         # both streams of the text read twice, four bytes written
        line.update(period_length_pass_GBps=round(gbps, 1), period_length_pass_fraction_of_copy_probe=round(gbps / probe, 3))
    for q in (d_in, d_out, d_back):
        ctx_on.dfree(q)
    ctx_on.close()
    ctx_off.close()
    print("LINE " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "period_step_bench.jsonl"))
    ap.add_argument("--child", default="")
    ap.add_argument("--off-first", action="store_true", help="make the BWTC_HIP_PERIODS=0 context first")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    only = [x for x in args.only.split(",") if x]
    for name in NAMES:
        if only and name not in only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--mib", str(args.mib), "--reps", str(args.reps), "--tag", args.tag] + (["--off-first"] if args.off_first else [])
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
