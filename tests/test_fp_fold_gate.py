"""The fresh ct_mul writer's gated canonical finish without a GPU (tests/cpp/fp_fold_gate_check.cpp):
csrc/fp127.hpp's fp_fold3_48_words + fp_fold3_48_rare + fp_fold3_48_finish, run as the writer runs
them, against fp_fold3_48 and the value mod p: sums of 0, p, p +- 1, 2^127, 2^127 + 1, top words
0x7FFFFFFF and 0 that are not p and not 0, 4,096 maximal addends and 10^6 random triples. Built as a
stand-alone host program with ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp_fold_gate_check(tmp_path):
    out = str(tmp_path / "fp_fold_gate_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
           "-I", os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "fp_fold_gate_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "fp_fold_gate_check: ok" in r.stdout
