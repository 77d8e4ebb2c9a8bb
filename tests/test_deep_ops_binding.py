"""pvac_hip_deep_route_count at the ABI and at the reference-side binding: the header declares it with the ABI
version still 3 and names the layer limit where ct_lincomb and compact say what they refuse, the library
exports it, the ctypes table of the Python package lists it with the arity of its prototype, the Python and
C++ surfaces exist, and tests/cpp/deep_ops_binding_check.cpp instantiates the adapter's deep-cipher flow next
to the REAL reference headers. CPU only; the compile is skipped where the reference is absent (the GPU box)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INC = "/root/reference/include"

PROTO = "int pvac_hip_deep_route_count(pvac_hip_ctx* ctx, uint64_t out[4]);"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return " ".join(f.read().replace(" * ", " ").split())


def test_header_declares_the_counter_and_names_the_limit():
    h = _read("include", "pvac_hip.h")
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    assert PROTO in h
    assert h.index("int pvac_hip_deep_path_count(") < h.index("int pvac_hip_deep_route_count(") < h.index("int pvac_hip_ct_mul_status(")
    # the three operations are no longer said to refuse at any limit
    assert "at any limit; an over-budget" not in h and "keep their 30000-layer refusals" not in h
    assert "PVAC_ENOSYS for a term above max(30000, the context's layer limit) layers" in h
    assert "more than max(30000, the context's layer limit) layers, 2^31 edges or more" in h
    assert "56 bytes per input edge" in h


def _lib():
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    assert os.path.exists(lib), "libpvac_hip.so not built (run __graft_entry__.build())"
    import pvac_hfhe_cppbyv_amd as pv
    return pv.load_library()


def test_load_library_binds_it_and_the_abi_is_still_3():
    L = _lib()
    assert L.pvac_hip_abi_version() == 3
    f = L.pvac_hip_deep_route_count
    assert f.restype is C.c_int and len(f.argtypes) == len(PROTO[PROTO.index("(") + 1:PROTO.rindex(")")].split(","))
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert f(None, out) == -22 and list(out) == [7, 7, 7, 7]   # a null context is refused, nothing is written


def test_python_and_adapter_surfaces_exist():
    import pvac_hfhe_cppbyv_amd as pv
    assert callable(pv.Engine.deep_route_counts)
    hpp = _read("include", "pvac_hip.hpp")
    assert "std::array<uint64_t, 4> deep_route_counts() const" in hpp
    assert hpp.index("uint32_t layer_limit() const") < hpp.index("deep_route_counts() const") < hpp.index("void set_enc_plan_limit(")


def test_documents_name_what_is_accepted():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = _read(doc)
        assert "deep_route_count" in text, doc
        assert "keep their 30000-layer refusals" not in text and "keep their 30,000-layer refusals" not in text, doc


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_INC, "pvac")), reason="reference headers not present")
def test_deep_ops_binding_compiles_against_reference_headers(tmp_path):
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib")
    assert os.path.exists(os.path.join(lib, "libpvac_hip.so")), "libpvac_hip.so not built (run __graft_entry__.build())"
    out = str(tmp_path / "deep_ops_binding_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-maes", "-mpclmul", "-msse4.1", "-D__HIP_PLATFORM_AMD__", "-I", REF_INC,
           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "deep_ops_binding_check.cpp"), "-o", out, "-pthread",
           "-L", lib, "-lpvac_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert os.path.exists(out)
