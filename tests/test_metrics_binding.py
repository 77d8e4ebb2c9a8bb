"""The metrics entry points (utils/metrics.hpp) at the ABI and at the reference-side binding: the header
declares pvac_hip_sigma_bytehist / pvac_hip_layer_gsum / pvac_hip_metrics_path_count with the ABI
version still 3, and tests/cpp/metrics_binding_check.cpp instantiates the adapter's sigma_shannon /
sigma_shannon_batch / agg_layer_gsum / layer_gsums_batch / dump_metrics on pvac:: types against the
REAL reference headers. CPU only; the compile is skipped where the reference is
absent (the GPU box)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INC = "/root/reference/include"


def test_header_declares_the_metrics_entry_points():
    with open(os.path.join(ROOT, "include", "pvac_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    flat = " ".join(h.split())
    for proto in ("int pvac_hip_sigma_bytehist(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* hist);",
                  "int pvac_hip_layer_gsum(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint64_t* gsum, uint32_t* status);",
                  "int pvac_hip_metrics_path_count(pvac_hip_ctx* ctx, uint64_t out[5]);"):
        assert proto in flat, proto
    assert "metrics (utils/metrics.hpp)" in h


def test_library_exports_the_metrics_entry_points():
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")
    import pvac_hfhe_cppbyv_amd as pv
    L = pv.load_library()
    assert L.pvac_hip_abi_version() == 3
    for name in ("pvac_hip_sigma_bytehist", "pvac_hip_layer_gsum", "pvac_hip_metrics_path_count"):
        assert getattr(L, name).restype is not None


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_INC, "pvac")), reason="reference headers not present")
def test_metrics_binding_compiles_against_reference_headers(tmp_path):
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libpvac_hip.so")):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")
    out = str(tmp_path / "metrics_binding_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-maes", "-mpclmul", "-msse4.1", "-D__HIP_PLATFORM_AMD__", "-I", REF_INC,
           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "metrics_binding_check.cpp"), "-o", out, "-pthread",
           "-L", lib, "-lpvac_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert os.path.exists(out)
