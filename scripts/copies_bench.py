#!/usr/bin/env python3
"""What BWTC_HIP_COPIES=1 -- copy rounds: whole copies at places that are no period look up past the copy in a doubling
round -- buys and costs, on one GPU: one JSON line per 256 MiB block.

Blocks: the generator's text with 16 copies of a 12 MiB piece of it behind 512-byte headers that differ; 1000 copies of a
200 KB piece at random places; `c3copies300` of scripts/r5/workloads.py (300 copies of a 10 KB piece); the real text with
its lines shuffled (24 copies of every line).  Controls: the plain generator's text, all zeros, period 9, and 1 MiB of text
256 times back to back -- a period above 4096, which the rule does not cover and which is reported as such.  Every block
is transformed on the device by two contexts -- with the switch and without -- --reps times each in rotating order, and
every result is taken back through the GPU inverse and compared with the block.  Not the back-to-back block's: the rows
of 256 copies' suffixes lie side by side, LF keeps a row's number modulo 64 over a quarter of the block, and the
inverse's walk from splitter to splitter (one thread, one row per 64) takes tens of millions of dependent loads there --
minutes per inverse.  That block's results are compared between the two contexts, bytes and LF powers.

Every block is measured by a child process of its own under a time limit (--limit seconds): a block that goes silent
costs its limit and its line, not the session.

A line holds, for "copies" and "off": ms_total and ms_sort of every repeat and their smallest, rounds, active_sum, route,
alg_bytes and sort_pass_items; Context.copies() with the switch; and, from one extra transform with the sorter's debug
lines, the three passes' own times per round (marks, flags, lengths) and the `copies:` line.

--parent DIR: a tree of the commit before the feature, built (DIR/bwtc_amd with its library).  The plain-text control is
then measured twice more, each time by a child that imports that tree (build "parent", "parent_again"): the spread between
the two is the parent build's own run-to-run spread, which the control with the switch must lie within.

Usage: scripts/copies_bench.py [--mib 256] [--reps 3] [--only NAME[,NAME]] [--tag TEXT] [--out FILE] [--limit 240] [--parent DIR]"""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("BWTC_BENCH_ROOT") or HERE          # (the tree whose bwtc_amd is measured: --parent sets it for one child)
sys.path.insert(0, ROOT)

PASSES_LINE = re.compile(r"copies: marks ([0-9.]+) ms, flags ([0-9.]+) ms, lengths ([0-9.]+) ms for (\d+) entries in (\d+) groups, \d+ suffixes: longest K (\d+)")
COPIES_LINE = re.compile(r"copies: \d+ passes.*")

NAMES = ["text_16_copies_of_12_MiB", "text_1000_copies_of_200_KB", "c3copies300", "shuffled_lines",
         "control_text", "control_zeros", "control_period_9", "not_covered_1_MiB_x_256_back_to_back"]
MODES = {"copies": "BWTC_HIP_COPIES", "off": None}


def workloads():
    spec = importlib.util.spec_from_file_location("workloads_r5", os.path.join(HERE, "scripts", "r5", "workloads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make(name, size):
    import numpy as np
    from bwtc_amd import synth
    if name == "control_zeros":
        return np.zeros(size, np.uint8)
    if name == "control_period_9":
        return np.tile(np.frombuffer(b"abcabcabd", np.uint8), size // 9 + 1)[:size].copy()
    if name == "c3copies300":
        return workloads().gen("c3copies300", size)[0]
    if name == "shuffled_lines":
        return workloads().gen("realtext", size)[0]
    if name == "not_covered_1_MiB_x_256_back_to_back":
        return workloads().gen("reptext", size)[0]
    d = synth.gen_text(size, 3).copy()
    rng = np.random.default_rng(16)
    if name == "text_16_copies_of_12_MiB":
        piece_len, head = size * 12 // 256, 512
        piece = d[:piece_len].copy()
        for i in range(16):
            at = i * (piece_len + head)
            d[at:at + head] = rng.integers(0, 256, head).astype(np.uint8)
            d[at + head:at + head + piece_len] = piece
    elif name == "text_1000_copies_of_200_KB":
        piece_len = max(64, size * 200 // (256 << 10))
        piece = d[54321:54321 + piece_len].copy()
        for at in rng.integers(0, size - piece_len, 1000):
            d[at:at + piece_len] = piece
    elif name != "control_text":
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
    os.environ.pop("BWTC_HIP_COPIES", None)
    if MODES[mode]:
        os.environ[MODES[mode]] = "1"
    ctx = hip.Context(0, size)
    os.environ.pop("BWTC_HIP_COPIES", None)
    return ctx


def child(name, args):
    """One block, measured in this process; the JSON line on stdout."""
    import numpy as np
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
    by_inverse = not name.startswith("not_covered")
    line["verified"] = "through the GPU inverse" if by_inverse else "the two contexts' bytes and LF powers against each other"
    seen = None
    for rep in range(args.reps):
        for m in modes[rep % len(modes):] + modes[:rep % len(modes)]:
            ctx = ctxs[m]
            lf, _ = ctx.bwt_block_device(d_in, d_out, size, 8)
            st = ctx.stats()
            runs[m].append({"ms_total": round(st.ms_total, 3), "ms_sort": round(st.ms_sort, 3), "rounds": st.rounds, "active_sum": st.active_sum,
                            "route": st.route, "alg_bytes": st.alg_bytes, "sort_pass_items": st.sort_pass_items})
            if by_inverse:
                ctx.inverse_bwt_block_device(d_out, d_back, size, lf)
                assert (ctx.to_host(d_back, size) == data).all(), (name, m, rep)
            else:
                got = (ctx.to_host(d_out, size), np.asarray(lf).copy())
                seen = seen or got
                assert (got[0] == seen[0]).all() and (got[1] == seen[1]).all(), (name, m, rep)
    for m, rr in runs.items():
        assert len({(r["rounds"], r["active_sum"], r["route"], r["alg_bytes"], r["sort_pass_items"]) for r in rr}) == 1, rr   # the block's, not the repeat's
        line[m] = {"ms_total": min(r["ms_total"] for r in rr), "ms_sort": min(r["ms_sort"] for r in rr),
                   "ms_total_all": [r["ms_total"] for r in rr], "ms_sort_all": [r["ms_sort"] for r in rr]}
        line[m].update({k: rr[0][k] for k in ("rounds", "active_sum", "route", "alg_bytes", "sort_pass_items")})
    for m, ctx in ctxs.items():
        if m != "copies":
            continue
        said = debug_lines(lambda: ctx.bwt_block_device(d_in, d_out, size, 8))
        line[m]["passes"] = [{"marks_ms": float(a), "flags_ms": float(b), "lengths_ms": float(c), "entries": int(e), "groups": int(g), "longest_K": int(k)}
                             for a, b, c, e, g, k in PASSES_LINE.findall(said)]
        s = COPIES_LINE.findall(said)
        line[m]["said"] = s[-1] if s else None
        rounds, passes, longest, first_depth = ctx.copies()
        line[m]["copies"] = {"rounds": rounds, "passes": passes, "longest_K": longest, "first_depth": first_depth}
    if name.startswith("not_covered"):
        line["note"] = "back-to-back copies of one piece are a period (1 MiB: above 4096), not covered by the rule"
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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "copy_rounds_bench.jsonl"))
    ap.add_argument("--parent", default="", help="a built tree of the commit before the feature: the plain-text control on it, twice")
    ap.add_argument("--child", default="")
    ap.add_argument("--modes", default="copies,off")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    only = [x for x in args.only.split(",") if x]
    for name in NAMES:
        if only and name not in only:
            continue
        if measure(name, args, "copies,off", args.tag) is None:
            return 1
        if name == "control_text" and args.parent:
            for tag in ("parent", "parent_again"):
                if measure(name, args, "off", tag, args.parent) is None:
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
