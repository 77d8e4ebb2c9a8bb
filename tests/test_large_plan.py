"""The general ct_mul path's host-side planning without a GPU (tests/cpp/large_plan_check.cpp):
csrc/large_plan.hpp's scratch layouts, shared-bucket test and sub-batch cut against values recorded
from the code before it moved there, built as a stand-alone host program with ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_large_plan_check(tmp_path):
    out = str(tmp_path / "large_plan_check")
    # hipcc, host side only: common.hpp declares device helpers a plain g++ does not know
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "large_plan_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "large_plan_check: ok" in r.stdout
