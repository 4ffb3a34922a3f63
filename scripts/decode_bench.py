#!/usr/bin/env python3
"""Decode-side figures of the 'H' coder on one GPU, one JSON line per workload.

For a 256 MiB C3 text block and a 256 MiB uniform-random block, both encoded by the product
(transform_and_encode):
  entropy_ms      device time of the entropy decode's kernels (bwtc_hip_huffman_decode statistics)
  entropy_wall_ms the same from the record's upload to the BWT bytes, the host-driven section chain
                  included; chain_host_ms = the difference, also per section
  inverse_ms      device time of the inverse transform inside decode_block_H
  decode_block_ms decode_block_H from the host record to the host bytes (the call synchronises)
  uncompress_s    `uncompress` end to end over a file of several blocks, on the default (GPU)
                  route and under BWTC_HIP_DECODE=host (serial HuffmanDecoder + GPU inverse)
Best of --reps runs each.  Usage: scripts/decode_bench.py [--mib 256] [--reps 3] [--out FILE]

With --prepr ppppp the line is that of the device postprocessor instead (a C3 text block precompressed by the
product): precompressed size, ms_device of the expansion, its algorithmic bytes (block read + expansion written +
the per-tile words, each once) over that time as a fraction of bwtc_hip_copy_probe, the host function's seconds
for the same block, and `uncompress` end to end over a four-block `-e H --prepr` file on the default route, under
BWTC_HIP_POSTPROCESS=host and under BWTC_HIP_DECODE=host, in alternating runs.

With --coder B (or b, u) the lines are those of the wavelet decode route: per block the host range decoder's
milliseconds, the device rebuild's (upload of the forest to BWT bytes) with its bit reads per second and its traffic
against bwtc_hip_copy_probe, the inverse, decode_block_W end to end, and `uncompress` over a several-block file on
the default route against BWTC_HIP_DECODE=host in alternating runs; the run fails unless the default route is faster
best against best by more than the spread of either side.

With --coder B --host-phases the lines are those of the serial host decoder alone (WaveletDecoder + upload + inverse +
download + write, the only route there was before the device route and what BWTC_HIP_DECODE=host still runs): per
file `uncompress` wall time and its phases as the debug tally prints them (decodeTreeBF and message summed over
sections, the inverse with its upload and download, the writes), for a one-block and a four-block file.  It uses
nothing but `compress`, `uncompress` and the tally line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bwtc_amd import hip, synth  # noqa: E402


def _best(fn, reps):
    best, out = None, None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best, out


def _uncompress(comp, dst, route, reps):
    env = dict(os.environ)
    env.pop("BWTC_HIP_DECODE", None)
    if route:
        env["BWTC_HIP_DECODE"] = route
    exe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    return _best(lambda: subprocess.run([exe, comp, dst], check=True, env=env), reps)[0]


def run_prepr(options, data, reps):
    size = data.size
    line = {"workload": "C3_text_prepr_" + options, "block_bytes": size}
    with hip.Context(0, 32 << 20) as ctx:
        g = hip.Grammar()
        pre = ctx.precompress(g, options, data)
        line.update(precompressed_bytes=int(pre.size), rules=g.rules, special_symbols=g.special_symbols)
        d_in, d_out = ctx.dmalloc(pre.size + 16), ctx.dmalloc(size + 16)
        ctx.to_device(d_in, pre)
        stats = []
        for _ in range(reps + 1):                            # first call: workspace
            assert ctx.postprocess_device(g, d_in, pre.size, d_out, size) == size
            stats.append(ctx.postprocess_stats())
        assert ctx.to_host(d_out, size).tobytes() == data.tobytes()
        ctx.dfree(d_in)
        ctx.dfree(d_out)
        st = min(stats[1:], key=lambda x: x["ms_device"])
        assert st["route"] == 1
        tiles = -(-pre.size // 4096)
        alg = pre.size + size + 2 * 4 * tiles                # run starts and offsets: one word per tile each
        probe = ctx.copy_probe(1 << 30, 5)
        gbps = alg / (st["ms_device"] * 1e-3) / 1e9
        t_host, back = _best(lambda: g.postprocess(pre, size), reps)
        assert back.tobytes() == data.tobytes()
        line.update(ms_device=round(st["ms_device"], 3), alg_bytes=int(alg), alg_GBps=round(gbps, 1), copy_probe_GBps=round(probe, 1),
                    fraction_of_copy_probe=round(gbps / probe, 3), host_postprocess_s=round(t_host, 3),
                    tokens=st["tokens"], pair_tokens=st["pair_tokens"], pool_bytes=st["pool_bytes"], launches=st["launches"],
                    workspace_bytes=st["workspace_bytes"])
    with tempfile.TemporaryDirectory() as tmp:
        src, comp = os.path.join(tmp, "in"), os.path.join(tmp, "in.bwtc")
        data.tofile(src)
        mem = int(size / 4 / 0.74 / 1e6) + 1                 # four precompressor blocks of 0.74 MB per MB
        subprocess.run([os.path.join(ROOT, "bwtc_amd", "host", "compress"), "-m", str(mem), "-e", "H", "--prepr", options, src, comp],
                       check=True, stdout=subprocess.DEVNULL)
        line["file_blocks"] = -(-size // int(0.74 * mem * 1e6))
        exe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
        routes = {"default": {}, "postprocess_host": {"BWTC_HIP_POSTPROCESS": "host"}, "decode_host": {"BWTC_HIP_DECODE": "host"}}
        times = {r: [] for r in routes}
        for _ in range(reps):                                # alternating runs
            for r, extra in routes.items():
                env = {k: v for k, v in os.environ.items() if k not in ("BWTC_HIP_POSTPROCESS", "BWTC_HIP_DECODE")}
                env.update(extra)
                dst = os.path.join(tmp, "out_" + r)
                t = time.perf_counter()
                subprocess.run([exe, comp, dst], check=True, env=env)
                times[r].append(round(time.perf_counter() - t, 3))
                assert open(dst, "rb").read() == data.tobytes(), r
                os.remove(dst)
    for r in routes:
        line["uncompress_%s_s" % r] = min(times[r])
        line["uncompress_%s_runs_s" % r] = times[r]
    spread = max(times["postprocess_host"]) - min(times["postprocess_host"])
    gain = min(times["postprocess_host"]) - min(times["default"])
    line.update(postprocess_host_spread_s=round(spread, 3), default_faster_by_s=round(gain, 3), default_faster_than_spread=bool(gain > spread))
    return line


def run_host_phases(coder, name, data, reps):
    import re
    size = data.size
    line = {"workload": name, "coder": coder, "bytes": size, "route": "BWTC_HIP_DECODE=host"}
    exe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    # what bwtc_hip_inverse_bwt_block does in one call, apart: the BWT bytes up from pageable memory, the inverse, the
    # block down into pageable memory
    with hip.Context(0, size) as ctx:
        bwt, lf, _ = ctx.bwt_block(data, 8)
        d_a, d_b = ctx.dmalloc(size + 16), ctx.dmalloc(size + 16)
        t_up = _best(lambda: ctx.to_device(d_a, bwt), reps + 1)[0]
        t_inv = _best(lambda: ctx.inverse_bwt_block_device(d_a, d_b, size, lf), reps + 1)[0]
        t_down, back = _best(lambda: ctx.to_host(d_b, size), reps + 1)
        assert back.tobytes() == data.tobytes()
        ctx.dfree(d_a)
        ctx.dfree(d_b)
        del bwt, back
        line["block"] = {"ms_upload_pageable": round(t_up * 1e3, 3), "ms_inverse": round(t_inv * 1e3, 3),
                         "ms_download_pageable": round(t_down * 1e3, 3)}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in")
        data.tofile(src)
        for blocks in (1, 4):
            comp, dst = os.path.join(tmp, "in%d.bwtc" % blocks), os.path.join(tmp, "out")
            mem = int(size / blocks / 0.185 / 1e6) + 1 + (blocks == 1)
            subprocess.run([os.path.join(ROOT, "bwtc_amd", "host", "compress"), "-m", str(mem), "-e", coder, src, comp],
                           check=True, stdout=subprocess.DEVNULL)
            best = None
            for _ in range(reps):
                env = dict(os.environ, BWTC_HIP_DECODE="host", BWTC_HIP_DEBUG="1")
                t = time.perf_counter()
                p = subprocess.run([exe, comp, dst], check=True, env=env, capture_output=True, text=True)
                wall = time.perf_counter() - t
                m = re.search(r"^wavelet host phases: ms_decode_tree ([0-9.]+) ms_message ([0-9.]+) ms_upload_inverse_download ([0-9.]+) "
                              r"ms_write ([0-9.]+)$", p.stderr, re.M)
                t2 = re.search(r"^wavelet decode: device (\d+) host (\d+)", p.stderr, re.M)
                assert m and t2 and int(t2.group(1)) == 0, p.stderr
                if best is None or wall < best["uncompress_s"]:
                    best = {"uncompress_s": round(wall, 3), "blocks": int(t2.group(2)), "ms_decode_tree": float(m.group(1)),
                            "ms_message": float(m.group(2)), "ms_upload_inverse_download": float(m.group(3)), "ms_write": float(m.group(4))}
            assert open(dst, "rb").read() == data.tobytes()
            os.remove(dst)
            best["message_share_of_wall"] = round(best["ms_message"] / (best["uncompress_s"] * 1e3), 3)
            best["decode_tree_share_of_wall"] = round(best["ms_decode_tree"] / (best["uncompress_s"] * 1e3), 3)
            line["file_%d_block" % blocks] = best
    return line


def run_wavelet(coder, name, data, reps, file_blocks_mb):
    size = data.size
    line = {"workload": name, "coder": coder, "block_bytes": size}
    with hip.Context(0, size) as ctx:
        ctx.wavelet_start(coder)
        rec, _ = ctx.transform_and_encode_wavelet(data, 8)
        line["record_bytes"] = int(rec.size)
        ctx.decode_block_W(hip.WaveletDecoder(coder), rec, cap=size)          # first call: workspace
        stats, walls = [], []
        for _ in range(reps):
            t = time.perf_counter()
            back = ctx.decode_block_W(hip.WaveletDecoder(coder), rec, cap=size)
            walls.append(time.perf_counter() - t)
            stats.append(ctx.wavelet_decode_stats())
        assert back.tobytes() == data.tobytes(), name
        st = min(stats, key=lambda x: x["ms_rebuild"])
        assert st["route"] == 1
        probe = ctx.copy_probe(1 << 30, 5)
        # words up, lines written and read once, run tables written and read, bytes written: the least the passes move
        alg = st["words"] * 8 * 3 + st["runs"] * (1 + 4 + 4) * 2 + size
        gbps = alg / (st["ms_rebuild"] * 1e-3) / 1e9
        line.update(ms_range_decode=round(min(s["ms_range_decode"] for s in stats), 3), ms_rebuild=round(st["ms_rebuild"], 3),
                    ms_inverse=round(st["ms_inverse"], 3), decode_block_ms=round(min(walls) * 1e3, 3),
                    sections=st["sections"], runs=st["runs"], nodes=st["nodes"], words=st["words"], bit_reads=st["bit_reads"],
                    bit_reads_per_s=round(st["bit_reads"] / (st["ms_rebuild"] * 1e-3), 0), launches=st["launches"],
                    alg_bytes=int(alg), alg_GBps=round(gbps, 1), copy_probe_GBps=round(probe, 1),
                    fraction_of_copy_probe=round(gbps / probe, 4), workspace_bytes=st["workspace_bytes"])
    with tempfile.TemporaryDirectory() as tmp:
        src, comp = os.path.join(tmp, "in"), os.path.join(tmp, "in.bwtc")
        data.tofile(src)
        subprocess.run([os.path.join(ROOT, "bwtc_amd", "host", "compress"), "-m", str(file_blocks_mb), "-e", coder, src, comp],
                       check=True, stdout=subprocess.DEVNULL)
        line["file_blocks"] = -(-size // int(0.185 * file_blocks_mb * 1e6))
        exe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
        times, tallies = {"default": [], "host": []}, {}
        for _ in range(reps):                                # alternating runs
            for r in ("default", "host"):
                env = {k: v for k, v in os.environ.items() if k != "BWTC_HIP_DECODE"}
                env["BWTC_HIP_DEBUG"] = "1"
                if r == "host":
                    env["BWTC_HIP_DECODE"] = "host"
                dst = os.path.join(tmp, "out_" + r)
                t = time.perf_counter()
                p = subprocess.run([exe, comp, dst], check=True, env=env, capture_output=True, text=True)
                times[r].append(round(time.perf_counter() - t, 3))
                tallies[r] = [ln for ln in p.stderr.splitlines() if ln.startswith("wavelet decode:")]
                if r == "default":
                    line["uncompress_default_worker"] = "".join(ln for ln in p.stderr.splitlines() if ln.startswith("wavelet worker:"))
                assert open(dst, "rb").read() == data.tobytes(), r
                os.remove(dst)
    for r in times:
        line["uncompress_%s_s" % r] = min(times[r])
        line["uncompress_%s_runs_s" % r] = times[r]
        line["uncompress_%s_tally" % r] = tallies[r][-1] if tallies[r] else ""
    spread = max(max(v) - min(v) for v in times.values())
    gain = min(times["host"]) - min(times["default"])
    line.update(spread_s=round(spread, 3), default_faster_by_s=round(gain, 3), default_faster_than_spread=bool(gain > spread))
    m = __import__("re").search(r"ms_range_decode ([0-9.]+) .* wall_ms ([0-9.]+)", line["uncompress_default_tally"])
    if m:
        line["range_decode_share_of_wall"] = round(float(m.group(1)) / float(m.group(2)), 3)
    return line


def run(name, data, reps, file_blocks_mb):
    size = data.size
    line = {"workload": name, "block_bytes": size}
    with hip.Context(0, size) as ctx:
        rec, _ = ctx.transform_and_encode(data, 8)
        line["record_bytes"] = int(rec.size)
        ctx.huffman_decode(rec)                              # first call: workspace
        ent = []
        for _ in range(reps):
            ctx.huffman_decode(rec)
            ent.append(ctx.huffman_decode_stats())
        best = min(ent, key=lambda x: x["ms_entropy_wall"])
        t, back = _best(lambda: ctx.decode_block_H(rec), reps)
        assert back.tobytes() == data.tobytes(), name
        st = ctx.huffman_decode_stats()
        line.update(entropy_ms=round(best["ms_entropy"], 3), entropy_wall_ms=round(best["ms_entropy_wall"], 3),
                    chain_host_ms=round(best["ms_chain_host"], 3),
                    chain_host_ms_per_section=round(best["ms_chain_host"] / max(best["sections"], 1), 4),
                    inverse_ms=round(st["ms_inverse"], 3),
                    decode_block_ms=round(t * 1e3, 3), decode_block_GBps=round(size / t / 1e9, 3),
                    sections=st["sections"], tiles=st["tiles"], map_entries_per_tile=round(st["map_entries"] / max(st["tiles"], 1), 2),
                    host_syncs=st["host_syncs"], retries=st["retries"], launches=st["launches"],
                    workspace_bytes_per_block_byte=round(st["workspace_bytes"] / size, 2))
    with tempfile.TemporaryDirectory() as tmp:
        src, comp = os.path.join(tmp, "in"), os.path.join(tmp, "in.bwtc")
        data.tofile(src)
        subprocess.run([os.path.join(ROOT, "bwtc_amd", "host", "compress"), "-m", str(file_blocks_mb), "-e", "H", src, comp],
                       check=True, stdout=subprocess.DEVNULL)
        line["file_blocks"] = -(-size // int(0.185 * file_blocks_mb * 1e6))
        outs = {}
        for route in ("", "host"):
            dst = os.path.join(tmp, "out_" + (route or "device"))
            line["uncompress_%s_s" % (route or "device")] = round(_uncompress(comp, dst, route, reps), 3)
            outs[route] = open(dst, "rb").read()
        assert outs[""] == outs["host"] == data.tobytes(), name
    line["uncompress_speedup"] = round(line["uncompress_host_s"] / line["uncompress_device_s"], 2)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--file-mem", type=int, default=400, help="compress -m for the multi-block file (0.185 MB blocks per MB)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--prepr", default=None, help="pre-stage options (ppppp): the device postprocessor's line instead")
    ap.add_argument("--coder", default="H", help="H (default), or B / b / u: the wavelet decode route's lines")
    ap.add_argument("--host-phases", action="store_true", help="with --coder B / b / u: the serial host decoder's phases only")
    ap.add_argument("--workloads", default="C3_text,uniform_random")
    a = ap.parse_args()
    size = a.mib << 20
    rng = np.random.default_rng(1)
    lines = []
    if a.prepr:
        lines.append(run_prepr(a.prepr, synth.gen_text(size, 3), a.reps))
        print(json.dumps(lines[0]), flush=True)
    for name, gen in () if a.prepr else (("C3_text", lambda: synth.gen_text(size, 3)),
                      ("uniform_random", lambda: rng.integers(0, 256, size, dtype=np.uint8))):
        if name not in a.workloads.split(","):
            continue
        if a.coder == "H":
            line = run(name, gen(), a.reps, a.file_mem)
        elif a.host_phases:
            line = run_host_phases(a.coder, name, gen(), a.reps)
        else:
            line = run_wavelet(a.coder, name, gen(), a.reps, a.file_mem)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    slower = [ln["workload"] for ln in lines if ln.get("default_faster_than_spread") is False]
    if slower:
        sys.exit("default route not faster than the host route by more than the spread: " + ", ".join(slower))


if __name__ == "__main__":
    main()
