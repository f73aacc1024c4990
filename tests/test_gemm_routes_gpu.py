"""GPU: tests/native/test_gemm_routes, one section per case -- the tile maps, the split-K slabs, the log-sum-exp strip partials, the output
edges and the weight-gradient kernel of the MFMA GEMMs against an integer reference, bit for bit (the driver's header says which launch
reaches which branch)."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("section", ["map", "slabs", "lse", "edges", "dw"])
def test_native_driver(section):
    path = os.path.join(ROOT, "build", "native", "test_gemm_routes")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "gemm_routes.mk"])
    out = subprocess.run(["timeout", "-k", "10", "300", path, section], capture_output=True, text=True)
    print("\n".join(line for line in out.stdout.splitlines() if "worst relative error" in line or "TESTS" in line))
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "GEMM ROUTES %s TESTS PASSED" % section in out.stdout and "host reference only" not in out.stdout
