#!/usr/bin/env python3
"""What the device models of the coders 'b' and 'u' (BWTC_HIP_LETTER_MODELS=1) change, on one GPU: one JSON line per
letter.

Workload: a stream of 256 MiB blocks of the generator's text (C3: seeds 3, 4, ... cycled over --blocks distinct blocks)
through bwtc_hip_wavelet_encode_device_begin / _end, --steps blocks per run, as bench.py feeds them (the next block's
upload under the transform, up to the context's depth of blocks under way).  Two contexts of ONE process, one made with
the switch and one without, take the same stream --reps times each in rotating order (after four untimed blocks each).  Every record is compared, by its
digest, between the two contexts and between the repeats.

A line holds, for "on" and "off" and every repeat: ms per block (first _begin to last _end over the blocks),
gpu_ms_per_step (what the feeding thread spends per block in the upload, the transform and _begin, bench.py's figure),
host CPU-seconds per block in the adaptive models and in the range coders (bwtc_hip_wavelet_host_clock, summed over the
worker threads), depth_needed, and the routes the blocks took.  The letter 'B' is the control: the switch must change
neither its routes nor the launches the library counts (the radix scatter's, bwtc_hip_get_kernel_timers) nor a byte.

Usage: scripts/letters_bench.py [--mib 256] [--steps 12] [--blocks 4] [--reps 3] [--letters b,u,B] [--threads 0] [--tag TEXT] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_stream(ctx, letter, pool, steps, threads, bufs):
    """One stream of `steps` blocks through `ctx` under `letter`: its figures and the records' digests."""
    size = pool[0].size
    d_in, d_out, ring = bufs
    depth = int(ctx.lib.bwtc_hip_wavelet_depth(ctx.handle))
    ctx.wavelet_start(letter)
    ctx.wavelet_routes(reset=True)
    ctx.reset_kernel_timers()
    m0, c0, b0 = ctx.wavelet_host_clock()
    pending, digests, feed_s = [], [], 0.0

    def collect():
        t, out = pending.pop(0)
        n = ctx.wavelet_encode_end(t)
        digests.append(hashlib.sha256(out[:n].tobytes()).hexdigest()[:20])

    ctx.to_device_async(d_in[0], pool[0])
    t_start = time.perf_counter()
    for i in range(steps):
        if len(pending) >= min(depth, len(ring) - 1):
            collect()
        t = time.perf_counter()
        ctx.copy_wait()
        ctx.to_device_async(d_in[(i + 1) % 2], pool[(i + 1) % len(pool)])
        lf, freqs = ctx.bwt_block_device(d_in[i % 2], d_out, size, 8)
        out = ring[i % len(ring)]
        pending.append((ctx.wavelet_encode_device_begin(d_out, size, lf, freqs, out, threads), out))
        feed_s += time.perf_counter() - t
    while pending:
        collect()
    wall = time.perf_counter() - t_start
    ctx.copy_wait()
    m1, c1, b1 = ctx.wavelet_host_clock()
    assert b1 - b0 == steps, (b0, b1, steps)
    r = ctx.wavelet_routes()
    return {"ms_per_block": round(1e3 * wall / steps, 2), "gpu_ms_per_step": round(1e3 * feed_s / steps, 2),
            "host_model_cpu_s_per_block": round((m1 - m0) / steps, 4), "host_coder_cpu_s_per_block": round((c1 - c0) / steps, 4),
            "depth_needed": ctx.wavelet_depth_needed(), "routes": {k: int(v) for k, v in r.items()},
            "scatter_launches": ctx.kernel_timers()["scatter_launches"]}, digests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--letters", default="b,u,B")
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "letter_models_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    from bwtc_amd import hip
    size = args.mib << 20

    def context(mode):
        os.environ.pop("BWTC_HIP_LETTER_MODELS", None)
        if mode == "on":
            os.environ["BWTC_HIP_LETTER_MODELS"] = "1"
        ctx = hip.Context(0, size)
        os.environ.pop("BWTC_HIP_LETTER_MODELS", None)
        return ctx

    ctxs = {"on": context("on"), "off": context("off")}
    pool = [hip.synth_into("t", 3 + j, ctxs["on"].host_alloc(size)) for j in range(max(1, args.blocks))]
    bufs = {}
    for mode, ctx in ctxs.items():
        bound = ctx.compress_bound(size)
        bufs[mode] = ([ctx.dmalloc(size + 64), ctx.dmalloc(size + 64)], ctx.dmalloc(size + 64),
                      [np.empty(bound, np.uint8) for _ in range(min(int(ctx.lib.bwtc_hip_wavelet_depth(ctx.handle)), args.steps) + 1)])
    for mode in ("on", "off"):                                # untimed: first use (allocations, the worker pool)
        run_stream(ctxs[mode], "B", pool, min(4, args.steps), args.threads, bufs[mode])
    for letter in [x for x in args.letters.split(",") if x]:
        reps = args.reps if letter != "B" else 1
        line = {"letter": letter, "block_bytes": size, "steps": args.steps, "distinct_blocks": len(pool), "reps": reps,
                "threads": args.threads, "on": [], "off": []}
        if args.tag:
            line["build"] = args.tag
        ref = None
        for rep in range(reps):
            for mode in (("on", "off") if rep % 2 == 0 else ("off", "on")):
                figures, digests = run_stream(ctxs[mode], letter, pool, args.steps, args.threads, bufs[mode])
                ref = ref or digests
                assert digests == ref, (letter, mode, rep)             # byte-equal records, between the contexts and the repeats
                line[mode].append(figures)
        line["records_equal"] = True
        off_ms = [f["ms_per_block"] for f in line["off"]]
        line["off_spread_ms_per_block"] = round(max(off_ms) - min(off_ms), 2)
        line["on_minus_off_ms_per_block"] = round(min(f["ms_per_block"] for f in line["on"]) - min(off_ms), 2)
        if letter == "B":
            a, b = line["on"][0], line["off"][0]
            line["control_ok"] = bool(a["routes"] == b["routes"] and a["scatter_launches"] == b["scatter_launches"])
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    for ctx in ctxs.values():
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
