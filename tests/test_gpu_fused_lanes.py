"""The 'B' coder's range-coder route with the lanes stepped inside the long chains
(BWTC_HIP_FUSED_LANES=1, the default with AVX-512) against the route of scalar tasks plus lane
engines (=0): whole records of 16 MiB text, 64 MiB DNA and 256 MiB text blocks, equal to each
other and to the oracle's records (their SHA-256 in tests/golden/bwt_large.json).

The switch is read when a context's host pipeline is made, at its first encoded block, so each
route runs in a child process of its own with the switch in its environment, and the pipeline's
BWTC_HIP_DEBUG line for every block says which route took it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("C3_text_16MiB", "C2_dna_64MiB", "C3_text_256MiB")

_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.getcwd())
from bwtc_amd import hip, synth
cases = {c["name"]: c for c in json.load(open(os.path.join("tests", "golden", "bwt_large.json")))["cases"]}
out = {}
ctx = hip.Context(device=0, max_block_size=(256 << 20) + 1024)
try:
    for name in sys.argv[1:]:
        c = cases[name]
        d = getattr(synth, c["gen"])(c["size"], c["seed"])
        ctx.wavelet_reset()
        ctx.wavelet_routes(reset=True)
        rec, _ = ctx.transform_and_encode_wavelet(d, c["sp"])
        r = ctx.wavelet_routes()
        out[name] = {"bytes": int(rec.size), "sha256": hashlib.sha256(rec.tobytes()).hexdigest(),
                     "models_device": int(r["models_device"]), "trees_device": int(r["trees_device"])}
finally:
    ctx.close()
print("RESULT " + json.dumps(out))
"""


def _records(fused):
    env = dict(os.environ, BWTC_HIP_FUSED_LANES=fused, BWTC_HIP_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _CHILD] + list(CASES), cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (fused, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    routes = [x for x in r.stderr.splitlines() if x.startswith("w-route:")]
    return json.loads(line[len("RESULT "):]), routes


def test_fused_lanes_route_gives_the_oracle_records():
    cases = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "bwt_large.json")))["cases"]}
    got = {}
    for fused in ("1", "0"):
        recs, routes = _records(fused)
        # one device-modelled block per case, and every one of them on the route asked for
        assert len(routes) == len(CASES), (fused, routes)
        marker = "with the lanes inside them" if fused == "1" else "lane engines at most"
        assert all(marker in x for x in routes), (fused, routes)
        for name in CASES:
            rec = recs[name]
            assert rec["models_device"] == rec["trees_device"] == 1, (name, fused, rec)
            assert rec["bytes"] == cases[name]["b_record_bytes"], (name, fused)
            assert rec["sha256"] == cases[name]["b_record_sha256"], (name, fused)
        got[fused] = recs
    assert got["1"] == got["0"]
