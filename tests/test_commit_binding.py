"""The reference-side binding of commit_ct compiles and links against the REAL
reference headers: tests/cpp/commit_binding_check.cpp instantiates the adapter's commit_ct /
commit_ct_batch on pvac:: types. CPU only; skipped where the reference is absent (the GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INC = "/root/reference/include"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_INC, "pvac")), reason="reference headers not present")
def test_commit_binding_compiles_against_reference_headers(tmp_path):
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libpvac_hip.so")):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")
    out = str(tmp_path / "commit_binding_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-maes", "-mpclmul", "-msse4.1", "-D__HIP_PLATFORM_AMD__", "-I", REF_INC,
           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "commit_binding_check.cpp"), "-o", out, "-pthread",
           "-L", lib, "-lpvac_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert os.path.exists(out)
