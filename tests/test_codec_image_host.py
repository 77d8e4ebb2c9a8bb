"""The device .ct codec's shared code without a GPU (tests/cpp/ct_image_host_check.cpp): csrc/ct_image.hpp,
the geometry, stream words, layer bytes and parse validation the kernels of k_ct_image.hip run,
instantiated on the host: every golden .ct file and the alignment sweep rebuilt granule by granule
against the host codec's bytes, and the validation on malformed spans. A stand-alone host program with
ASan + UBSan, run as a child process."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ct_image_host_check(tmp_path):
    out = str(tmp_path / "ct_image_host_check")
    csrc = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc")
    # hipcc, host side only: ct_image.hpp carries __host__ __device__ functions
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "ct_image_host_check.cpp"), os.path.join(csrc, "ct_codec.cpp"),
           "-pthread", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "**", "*.ct"), recursive=True))
    assert len(files) >= 40
    r = subprocess.run([out] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"ct_image_host_check: ok ({len(files)} files" in r.stdout
