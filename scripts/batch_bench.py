#!/usr/bin/env python3
"""Batched block transform against the loop of single transforms, on one GPU, one JSON line per measurement.

For every block size, batch size and input kind the blocks lie in device memory; measured are
  batch   one bwtc_hip_bwt_blocks_device call over all of them: wall time around the call (it ends in a device
          synchronise) and device time (bwtc_hip_batch_stats.ms_total, HIP events), with rounds and host waits
  loop    bwtc_hip_bwt_block_device block by block, the only way before the batched call: wall time around the
          loop and the sum of the blocks' device times (bwtc_hip_stats.ms_total)
each --reps times after a warm-up, on two contexts (one per side), the two sides in alternating order from repeat to
repeat.  A line carries every repeat, the best, the median and the spread (max - min) of both sides, and `wins`:
the batch's worst repeat beats the loop's best by more than nothing, i.e. the margin best-against-best exceeds the
larger spread.  Combinations whose strides do not fit the context (k * S above 2^28 positions) are skipped and say so.

--loop-only measures the loop alone and --lib PATH loads another build of the library: together they run the loop
on the parent commit's build, which has no batched call.
--cli adds `compress -m 1` and `-m 5` wall times over a text file with BWTC_HIP_BATCH set and without, alternating.

Usage: scripts/batch_bench.py [--reps 5] [--out profiles/batch_bwt_bench.jsonl] [--loop-only] [--lib PATH] [--cli]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bwtc_amd import hip, synth  # noqa: E402

POSITIONS = 1 << 28
SIZES = [4000, 64 << 10, 185000, 1 << 20, 4 << 20]
COUNTS = [16, 256, 4096]
KINDS = ["random", "text", "zeros"]


def make_input(kind, nbytes, seed=1):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    if kind == "text":
        return np.ascontiguousarray(synth.gen_text(nbytes, 3)[:nbytes])
    return np.zeros(nbytes, np.uint8)


def stride_log2(size):
    k = 0
    while (1 << k) < size + 1:
        k += 1
    return k


def summary(values):
    return {"runs": [round(v, 4) for v in values], "best": round(min(values), 4), "median": round(statistics.median(values), 4),
            "spread": round(max(values) - min(values), 4)}


def measure(ctx_batch, ctx_loop, data, size, count, reps, loop_only):
    pitch = (size + 15) // 16 * 16
    offsets = [i * pitch for i in range(count)]
    sizes = [size] * count
    buf = np.zeros(pitch * count, np.uint8)
    for i, off in enumerate(offsets):
        buf[off:off + size] = data[i * size:(i + 1) * size]
    owner = ctx_loop
    d_in, d_out = owner.dmalloc(buf.size), owner.dmalloc(buf.size)
    owner.to_device(d_in, buf)
    res = {"batch_wall": [], "batch_dev": [], "loop_wall": [], "loop_dev": []}
    extra = {}

    def run_batch(keep):
        t0 = time.perf_counter()
        ctx_batch.bwt_blocks_device(d_in, d_out, offsets, sizes, 8)
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx_batch.batch_stats()
        if keep:
            res["batch_wall"].append(wall)
            res["batch_dev"].append(float(st["ms_total"]))
            extra.update(rounds=st["rounds"], host_waits=st["host_waits"])

    def run_loop(keep):
        dev = 0.0
        t0 = time.perf_counter()
        for off in offsets:
            ctx_loop.bwt_block_device(d_in + off, d_out + off, size, 8)
            dev += float(ctx_loop.stats().ms_total)
        wall = (time.perf_counter() - t0) * 1e3
        if keep:
            res["loop_wall"].append(wall)
            res["loop_dev"].append(dev)

    try:
        for r in range(reps + 1):                       # repeat 0 is the warm-up
            order = [run_loop] if loop_only else ([run_batch, run_loop] if r % 2 else [run_loop, run_batch])
            for fn in order:
                fn(r > 0)
    finally:
        owner.dfree(d_in)
        owner.dfree(d_out)
    line = {k: summary(v) for k, v in res.items() if v}
    line.update(extra)
    if not loop_only:
        b, l = line["batch_wall"], line["loop_wall"]
        line["speedup_best"] = round(l["best"] / b["best"], 3)
        line["margin_ms"] = round(l["best"] - b["best"], 4)
        line["wins"] = bool(l["best"] - b["best"] > max(b["spread"], l["spread"]))
    return line


def cli_times(out, reps):
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    data = make_input("text", 48_000_000)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.bin")
        data.tofile(src)
        for mem in (1, 5):
            for coder in ("H", "B"):
                times = {"plain": [], "batched": []}
                streams = {}
                for r in range(reps + 1):
                    names = ["plain", "batched"] if r % 2 else ["batched", "plain"]
                    for name in names:
                        env = {k: v for k, v in os.environ.items() if not k.startswith("BWTC_HIP_BATCH")}
                        if name == "batched":
                            env["BWTC_HIP_BATCH"] = "64"
                        dst = os.path.join(tmp, name + ".bwtc")
                        t0 = time.perf_counter()
                        subprocess.run([exe, "-m", str(mem), "-e", coder, src, dst], check=True, env=env, timeout=600)
                        if r > 0:
                            times[name].append(time.perf_counter() - t0)
                        with open(dst, "rb") as f:
                            streams[name] = f.read()
                assert streams["plain"] == streams["batched"], "the batched stream differs"
                line = {"what": "compress", "mem": mem, "coder": coder, "input_bytes": int(data.size), "batch": 64,
                        "plain_s": summary(times["plain"]), "batched_s": summary(times["batched"])}
                emit(out, line)


def tolerate_missing_batch_calls():
    """--loop-only: a build from before the batched call has to load too, so its four missing names resolve to a stub
    that takes the argument types and is never called."""
    import ctypes
    missing = ("bwtc_hip_bwt_blocks", "bwtc_hip_bwt_blocks_device", "bwtc_hip_batch_stats_get", "bwtc_hip_test_batch_keys")

    class Stub:
        argtypes = None
        restype = None

    class Library(ctypes.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if name in missing:
                    return Stub()
                raise

    ctypes.CDLL = Library


def emit(out, line):
    text = json.dumps(line)
    print(text, flush=True)
    out.write(text + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bwt_bench.jsonl"))
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--counts", type=int, nargs="*", default=COUNTS)
    ap.add_argument("--kinds", nargs="*", default=KINDS)
    args = ap.parse_args()
    if args.lib:
        hip.LIB_PATH = os.path.abspath(args.lib)
    if args.loop_only:
        tolerate_missing_batch_calls()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        ctx_batch = None if args.loop_only else hip.Context(0, POSITIONS - 1)
        ctx_loop = hip.Context(0, max(args.sizes))
        inputs = {}
        for size in args.sizes:
            for count in args.counts:
                fits = (count << stride_log2(size)) <= POSITIONS
                for kind in args.kinds:
                    head = {"what": "transform", "build": args.label, "size": size, "count": count, "kind": kind}
                    if not fits:
                        emit(out, dict(head, skipped="k * S above 2^28 positions"))
                        continue
                    need = size * count
                    if kind not in inputs or inputs[kind].size < need:
                        inputs[kind] = make_input(kind, need)
                    emit(out, dict(head, **measure(ctx_batch, ctx_loop, inputs[kind], size, count, args.reps, args.loop_only)))
        if ctx_batch:
            ctx_batch.close()
        ctx_loop.close()
        if args.cli:
            cli_times(out, max(2, args.reps // 2))


if __name__ == "__main__":
    main()
