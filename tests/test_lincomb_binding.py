"""The binding of ct_lincomb, CPU only: include/pvac_hip.h declares and libpvac_hip.so exports the four
entry points; the adapter's ct_sum / ct_lincomb / ct_lincomb_batch compile and link against the REAL
reference headers (tests/cpp/lincomb_binding_check.cpp; skipped where the reference is absent); and the
adapter's flattening of a call's ragged lists (tests/cpp/lincomb_flatten_check.cpp) holds under
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INC = "/root/reference/include"
LIBDIR = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib")
SYMS = ("pvac_hip_ct_lincomb_plan", "pvac_hip_ct_lincomb_exec", "pvac_hip_ct_lincomb_path_count",
        "pvac_hip_ct_lincomb_status")


def built():
    if not os.path.exists(os.path.join(LIBDIR, "libpvac_hip.so")):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")


def test_header_declares_and_library_exports_lincomb():
    built()
    with open(os.path.join(ROOT, "include", "pvac_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = C.CDLL(os.path.join(LIBDIR, "libpvac_hip.so"))
    for s in SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), s
        assert hasattr(lib, s), s
    assert re.search(r"#define\s+PVAC_TERM_SCALE\s+0x1u", text)
    assert re.search(r"typedef struct pvac_lincomb\s*\{[^}]*seg_off[^}]*term[^}]*scale[^}]*flags[^}]*\}\s*pvac_lincomb;", text)
    assert re.search(r"#define\s+PVAC_HIP_ABI_VERSION\s+3\b", text)


def test_python_binding_has_lincomb():
    built()
    import pvac_hfhe_cppbyv_amd as pv
    lib = pv.load_library()
    for s in SYMS:
        assert getattr(lib, s).argtypes is not None, s
    assert C.sizeof(pv.Lincomb) == 48 and pv.TERM_SCALE == 1
    for m in ("ct_lincomb", "ct_sum", "ct_lincomb_path_counts"):
        assert callable(getattr(pv.Engine, m))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_INC, "pvac")), reason="reference headers not present")
def test_lincomb_binding_compiles_against_reference_headers(tmp_path):
    built()
    out = str(tmp_path / "lincomb_binding_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-maes", "-mpclmul", "-msse4.1", "-D__HIP_PLATFORM_AMD__", "-I", REF_INC,
           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "lincomb_binding_check.cpp"), "-o", out, "-pthread",
           "-L", LIBDIR, "-lpvac_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert os.path.exists(out)


def test_lincomb_flatten_under_sanitizers(tmp_path):
    built()
    out = str(tmp_path / "lincomb_flatten_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "lincomb_flatten_check.cpp"), "-o", out, "-pthread",
           "-L", LIBDIR, "-lpvac_hip", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "lincomb_flatten_check: ok" in r.stdout
