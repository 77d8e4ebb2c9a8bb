"""pvac_hip_batch_gather's work split without a GPU (tests/cpp/gather_tiles_check.cpp):
csrc/gather_tiles.hpp's tiles, tile -> cipher search, runs and 16-byte split, built as a stand-alone host
program with ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_tiles_check(tmp_path):
    out = str(tmp_path / "gather_tiles_check")
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "gather_tiles_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "gather_tiles_check: ok" in r.stdout
