#!/usr/bin/env python3
"""What the period steps above 4096 (BWTC_HIP_LONG_PERIODS=1) buy, on one GPU: one JSON line per 256 MiB block.

Blocks: one period of 8192 and of 65 536 random bytes; 1 MiB of the generator's text 256 times back to back, as shipped
and with BWTC_HIP_COPIES=1 in both contexts; the generator's text with one 64 MiB stretch of period 7680 (a bitmap row
of 1920 x 4 bytes).  Controls, which hold no long period: the generator's plain text, zeros, period 9, fixed-width
records, period 4096.  Every block is transformed on the device by two contexts of one process, one with the switch and
one without, --reps times each in alternating order, and every result is taken back through the GPU inverse and compared
with the block (the back-to-back block's results are compared between the two contexts instead: its inverse takes
minutes).  The conventions are scripts/periods_bench.py's: a child process per block under a time limit, the
smallest repeat reported beside all of them.

A line holds, for "on" and "off": ms_total and ms_sort of every repeat and their smallest, rounds, active_sum and route;
what bwtc_hip_period_get says with the switch; the finder's two sweeps, the period-length pass and the trial passes (the
division's among them) by the sorter's debug lines, from one extra transform.  For a control the line also says whether
the acceptance rule holds: the smallest time with the switch not above the largest repeat without it, equal rounds and
route.

Usage: scripts/long_periods_bench.py [--mib 256] [--reps 5] [--only NAME[,NAME]] [--tag TEXT] [--out FILE] [--limit 240] [--off-first]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASS_LINE = re.compile(r"periods: the period-length pass took ([0-9.]+) ms")
TRIAL_LINE = re.compile(r"periods: a trial pass \(no lengths stored\) took ([0-9.]+) ms for \d+ suffixes, period (\d+)")
SWEEP1_LINE = re.compile(r"periods: sweep 1 of the long finder .* took ([0-9.]+) ms, (\d+) coarse bins")
SWEEP2_LINE = re.compile(r"periods: sweep 2 of the long finder took ([0-9.]+) ms for (\d+) coarse bins")
VOTE_LINE = re.compile(r"periods: the vote kernel took ([0-9.]+) ms for (\d+) entries")
SAID_LINE = re.compile(r"periods: period .*")

NAMES = ["period_8192_random", "period_65536_random", "text_1MiB_x256", "text_1MiB_x256_copies", "text_one_quarter_period_7680",
         "control_text", "control_zeros", "control_period_9", "control_records_64_with_8_random", "control_period_4096_random"]


def make(name, size):
    import numpy as np
    from bwtc_amd import synth
    rng = np.random.default_rng(5)

    def tiled(unit):
        return np.tile(unit, size // unit.size + 1)[:size].copy()

    if name == "period_8192_random":
        return tiled(rng.integers(0, 256, 8192).astype(np.uint8))
    if name == "period_65536_random":
        return tiled(rng.integers(0, 256, 65536).astype(np.uint8))
    if name in ("text_1MiB_x256", "text_1MiB_x256_copies"):
        return tiled(synth.gen_text(1 << 20, 3))
    if name == "text_one_quarter_period_7680":
        d = synth.gen_text(size, 3).copy()
        d[size // 4:size // 2] = tiled(rng.integers(0, 256, 7680).astype(np.uint8))[:size // 4]
        return d
    if name == "control_text":
        return synth.gen_text(size, 3)
    if name == "control_zeros":
        return np.zeros(size, np.uint8)
    if name == "control_period_9":
        return tiled(np.frombuffer(b"abcabcabd", np.uint8))
    if name == "control_records_64_with_8_random":
        d = tiled(rng.integers(0, 256, 64).astype(np.uint8)).reshape(-1)
        rec = d[:size // 64 * 64].reshape(-1, 64)
        rec[:, 20:28] = rng.integers(0, 256, (rec.shape[0], 8)).astype(np.uint8)
        return d
    if name == "control_period_4096_random":
        return tiled(rng.integers(0, 256, 4096).astype(np.uint8))
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
    import numpy as np
    from bwtc_amd import hip
    size = args.mib << 20
    if name.endswith("_copies"):
        os.environ["BWTC_HIP_COPIES"] = "1"                   # in both contexts: what the new switch changes under it

    def context(mode):
        os.environ.pop("BWTC_HIP_LONG_PERIODS", None)
        if mode == "on":
            os.environ["BWTC_HIP_LONG_PERIODS"] = "1"
        ctx = hip.Context(0, size)
        os.environ.pop("BWTC_HIP_LONG_PERIODS", None)
        return ctx

    if args.off_first:
        ctx_off = context("off")
        ctx_on = context("on")
    else:
        ctx_on = context("on")
        ctx_off = context("off")
    d_in, d_out, d_back = (ctx_on.dmalloc(size + 64) for _ in range(3))
    data = make(name, size)
    line = {"block": name, "block_bytes": size, "reps": args.reps, "first_context": "off" if args.off_first else "on"}
    if args.tag:
        line["build"] = args.tag
    runs = {"on": [], "off": []}
    # (not through the inverse for the back-to-back block: the rows of 256 copies' suffixes lie side by side and the inverse's
    # walk from splitter to splitter takes minutes there, scripts/copies_bench.py; its results are compared between the contexts)
    between, ref = name.startswith("text_1MiB_x256"), None
    ctx_on.to_device(d_in, data)                              # (the transform leaves its input as it is)
    for rep in range(args.reps):
        for mode, ctx in (("on", ctx_on), ("off", ctx_off)) if rep % 2 == 0 else (("off", ctx_off), ("on", ctx_on)):
            lf, _ = ctx.bwt_block_device(d_in, d_out, size, 8)
            st = ctx.stats()
            runs[mode].append({"ms_total": round(st.ms_total, 3), "ms_sort": round(st.ms_sort, 3), "rounds": st.rounds,
                               "active_sum": st.active_sum, "route": st.route})
            if between:
                got = (ctx.to_host(d_out, size).copy(), np.array(lf).copy())
                ref = ref or got
                assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all(), (name, mode, rep)
            else:
                ctx.inverse_bwt_block_device(d_out, d_back, size, lf)
                assert (ctx.to_host(d_back, size) == data).all(), (name, mode, rep)
    for mode, rr in runs.items():
        assert len({(r["rounds"], r["active_sum"], r["route"]) for r in rr}) == 1, rr       # the route is the block's, not the repeat's
        line[mode] = {"ms_total": min(r["ms_total"] for r in rr), "ms_sort": min(r["ms_sort"] for r in rr),
                      "ms_total_all": [r["ms_total"] for r in rr], "ms_sort_all": [r["ms_sort"] for r in rr],
                      "rounds": rr[0]["rounds"], "active_sum": rr[0]["active_sum"], "route": rr[0]["route"]}
    if name.startswith("control_"):
        line["control_ok"] = bool(line["on"]["ms_total"] <= max(line["off"]["ms_total_all"]) and line["on"]["rounds"] == line["off"]["rounds"]
                                  and line["on"]["route"] == line["off"]["route"])
    if name.endswith("_copies"):
        line["copies_on"], line["copies_off"] = list(ctx_on.copies()), list(ctx_off.copies())
    said = debug_lines(ctx_on, d_in, d_out, size)
    p, longest, votes, depth = ctx_on.period()
    line["period_get"] = {"p": p, "longest": longest, "votes": votes, "step_depth": depth}
    m = SAID_LINE.search(said)
    line["said"] = m.group(0) if m else None
    m = VOTE_LINE.search(said)
    line["vote_entries"] = int(m.group(2)) if m else None
    m = SWEEP1_LINE.search(said)
    line["sweep1_ms"], line["coarse_bins"] = (float(m.group(1)), int(m.group(2))) if m else (None, None)
    m = SWEEP2_LINE.search(said)
    line["sweep2_ms"] = float(m.group(1)) if m else None
    m = VOTE_LINE.search(debug_lines(ctx_off, d_in, d_out, size))
    line["vote_kernel_ms_off"] = float(m.group(1)) if m else None
    line["period_length_pass_ms"] = [float(x) for x in PASS_LINE.findall(said)]
    line["trial_pass_ms"] = [[float(ms), int(q)] for ms, q in TRIAL_LINE.findall(said)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_period_step_bench.jsonl"))
    ap.add_argument("--child", default="")
    ap.add_argument("--off-first", action="store_true", help="make the context without the switch first")
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
