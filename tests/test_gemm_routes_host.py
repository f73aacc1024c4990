"""CPU: the host mode of tests/native/test_gemm_routes -- its generator's exactness, the lse input condition, the refusals of the GEMM
launchers, and that its judging reports an element one unit off, swapped tiles, a shifted slab range, a strip that takes in column N_real
and a written guard byte.  No HIP call is made; hipcc cross-compiles the driver."""
import os
import subprocess

from conftest import ROOT


def test_native_driver_host_mode():
    path = os.path.join(ROOT, "build", "native", "test_gemm_routes")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "gemm_routes.mk"])
    out = subprocess.run([path, "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "GEMM ROUTES TESTS PASSED" in out.stdout and "host reference only" in out.stdout
