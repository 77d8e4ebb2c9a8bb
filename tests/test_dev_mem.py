"""The runtime's owning device buffers and device guard without a GPU (tests/cpp/dev_mem_check.cpp):
csrc/dev_mem.hpp against a fake allocator that counts bytes, can fail the k-th allocation and keeps a
map of live blocks, built with ASan + UBSan and without the HIP runtime library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_mem_check(tmp_path):
    out = str(tmp_path / "dev_mem_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
           "-I", os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "dev_mem_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "dev_mem_check: ok" in r.stdout
