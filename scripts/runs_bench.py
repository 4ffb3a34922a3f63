#!/usr/bin/env python3
"""What the suffix sorter's run step buys, on one GPU: one JSON line per 256 MiB block.

Blocks with long runs of one byte (zeros, 0xFF, the generator's text with one 64 MiB zero run, with 1000 runs of
64 KiB, an image-like block of 1 MiB of text and 3 MiB of zeros in turn) and controls without (period 9, 1 MiB of
text 256 times, the plain generator text).  Every block is transformed on the device by two contexts of this
process, one as shipped (BWTC_HIP_RUNS=1) and one with BWTC_HIP_RUNS=0, --reps times each in alternating order, and
every result is taken back through the GPU inverse and compared with the block.

A line holds, for "on" and "off": ms_total and ms_sort of every repeat and their smallest, rounds, active_sum and
route; the run-length pass's own time (the sorter's debug line, from one extra transform), its traffic of 6 bytes
per byte over that time and bwtc_hip_copy_probe beside it; for the all-zero block the reference's divsufsort on this
host over a 64 MiB block of zeros (oracle/_ref, where it was built).

Usage: scripts/runs_bench.py [--mib 256] [--reps 5] [--only NAME[,NAME]] [--tag TEXT] [--out FILE]
(BWTC_HIP_LIB=<another build's libbwtc_hip.so> measures that build: --tag names it in the lines.)"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from bwtc_amd import hip, synth  # noqa: E402

PASS_LINE = re.compile(r"runs: the run-length pass took ([0-9.]+) ms")


def blocks(size):
    """(name, maker) of every block; the text is made once."""
    mib = 1 << 20
    text = {}

    def gen():
        if "t" not in text:
            text["t"] = synth.gen_text(size, 3)
        return text["t"]

    def one_run():
        d = gen().copy()
        a = size // 4
        d[a:a + size // 4] = 0
        return d

    def many_runs():
        d = gen().copy()
        ln = max(1, size // 4096)                        # 64 KiB at 256 MiB
        step = size // 1000
        for i in range(1000):
            d[i * step:i * step + min(ln, step // 2)] = 0
        return d

    def image():
        d = gen().copy()
        for a in range(0, size, 4 * mib):
            d[a + mib:a + 4 * mib] = 0
        return d

    def copies():
        piece = gen()[:mib]
        return np.tile(piece, -(-size // mib))[:size].copy()

    return [("zeros", lambda: np.zeros(size, np.uint8)),
            ("ff", lambda: np.full(size, 255, np.uint8)),
            ("text_one_quarter_zero_run", one_run),
            ("text_1000_runs", many_runs),
            ("image_1MiB_text_3MiB_zeros", image),
            ("control_period_9", lambda: np.tile(np.frombuffer(b"abcabcabd", np.uint8), size // 9 + 1)[:size].copy()),
            ("control_text", gen),
            ("control_1MiB_text_copies", copies)]                # (last: its check through the inverse is the slowest step by far)


def pass_time(ctx, d_in, d_out, size):
    """The run-length pass's milliseconds from the sorter's debug line (None: the block launched none)."""
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
        m = PASS_LINE.search(tmp.read().decode("utf-8", "replace"))
    return float(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "run_ranks_bench.jsonl"))
    args = ap.parse_args()
    size = args.mib << 20
    only = [x for x in args.only.split(",") if x]

    os.environ.pop("BWTC_HIP_RUNS", None)
    ctx_on = hip.Context(0, size)
    os.environ["BWTC_HIP_RUNS"] = "0"
    ctx_off = hip.Context(0, size)
    del os.environ["BWTC_HIP_RUNS"]
    probe = ctx_on.copy_probe(1 << 30, 5)
    d_in, d_out, d_back = (ctx_on.dmalloc(size + 64) for _ in range(3))
    for name, make in blocks(size):
        if only and name not in only:
            continue
        data = make()
        line = {"block": name, "block_bytes": size, "reps": args.reps, "copy_probe_GBps": round(probe, 1)}
        if args.tag:
            line["build"] = args.tag
        runs = {"on": [], "off": []}
        ctx_on.to_device(d_in, data)                          # (the transform leaves its input as it is)
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
        ms = pass_time(ctx_on, d_in, d_out, size)
        line["run_length_pass_ms"] = ms
        if ms:
            gbps = 6.0 * size / (ms * 1e-3) / 1e9
            line.update(run_length_pass_GBps=round(gbps, 1), run_length_pass_fraction_of_copy_probe=round(gbps / probe, 3))
        if name == "zeros":
            import oracle_lib
            if oracle_lib.ref() is not None:
                z = np.zeros(64 << 20, np.uint8)
                took = []
                for _ in range(3):
                    t = time.perf_counter()
                    oracle_lib.ref_bwt_block(z, 8)
                    took.append(time.perf_counter() - t)
                line["reference_divsufsort_64MiB_zeros_s_all"] = [round(x, 3) for x in took]
                line["reference_divsufsort_64MiB_zeros_s"] = round(min(took), 3)
                line["reference_divsufsort_64MiB_zeros_GBps"] = round(z.size / min(took) / 1e9, 4)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:                        # (line by line: a run cut short keeps what it measured)
            f.write(json.dumps(line) + "\n")
    for p in (d_in, d_out, d_back):
        ctx_on.dfree(p)
    ctx_on.close()
    ctx_off.close()


if __name__ == "__main__":
    main()
