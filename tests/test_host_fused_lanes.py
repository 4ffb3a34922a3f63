"""The 'B' coder's range-coder lanes stepped inside the long chains (runChainsWithLanes,
bwtc_amd/csrc/wavelet_rc.cpp) against every chain coded alone by the scalar loop: the C++ program
tests/cpp/fused_lanes_test.cpp, built by the host Makefile.  Host code only, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_lanes_bytes_equal_scalar_chains():
    exe = os.path.join(ROOT, "tests", "cpp", "fused_lanes_test")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "bwtc_amd", "host"), "../../tests/cpp/fused_lanes_test"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] in ("ok", "skip: no AVX-512"), r.stdout
