"""The fresh ct_mul kernel's limb accumulators without a GPU (tests/cpp/fp_limbs_check.cpp):
csrc/fp127.hpp's fp_split3_48 / fp_fold3_48 against the sum mod p and the 44/44/40 pair, the cell id's
bits under 4,096 maximal addends, and fp_mul_fold1f against fp_mul_fold1, built as a stand-alone host
program with ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp_limbs_check(tmp_path):
    out = str(tmp_path / "fp_limbs_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
           "-I", os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "fp_limbs_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "fp_limbs_check: ok" in r.stdout
