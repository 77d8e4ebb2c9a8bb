"""commit_ct's message feeder without a GPU (tests/cpp/commit_host_check.cpp): csrc/commit_msg.hpp, the
code every lane of k_commit_ct runs, instantiated on the host over the fixture files (read through
csrc/ct_codec.cpp) against the digests the reference minted, and over a sweep of message lengths,
field values and sigma widths against a byte-wise SHA-256. A stand-alone host program with
ASan + UBSan."""
import os
import subprocess

from commit_cases import fixture_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_commit_host_check(tmp_path):
    out = str(tmp_path / "commit_host_check")
    csrc = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc")
    # hipcc, host side only: sha256.hpp and commit_msg.hpp carry __host__ __device__ functions
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "commit_host_check.cpp"), os.path.join(csrc, "ct_codec.cpp"),
           "-pthread", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    man, cases = fixture_cases()
    assert len(cases) == 24
    args = [f"{path}:{int(sig)}:{digest}" for path, sig, digest in cases]
    r = subprocess.run([out, str(man["canon_tag"]), man["H_digest"]] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "commit_host_check: ok (24 fixture digests" in r.stdout
