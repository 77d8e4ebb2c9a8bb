"""The host runtime's exception boundary and plan scratch without a GPU (tests/cpp/ctx_check.cpp):
csrc/ctx.hpp itself against the fake allocator of tests/cpp/fake_hip.hpp, built as a stand-alone host
program with ASan + UBSan and without the HIP runtime library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctx_check(tmp_path):
    out = str(tmp_path / "ctx_check")
    # hipcc, host side only: ctx.hpp holds the context, whose members are types of common.hpp, and that
    # header declares device helpers a plain g++ does not know; -no-hip-rt keeps libamdhip64 out
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-Wall", "-x", "hip", "--cuda-host-only",
           "--offload-arch=gfx950", "-no-hip-rt", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "ctx_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    ldd = subprocess.run(["ldd", out], capture_output=True, text=True, timeout=60)
    assert "amdhip64" not in ldd.stdout, ldd.stdout
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ctx_check: ok" in r.stdout
