"""pvac_hip_batch_gather at the ABI and at the reference-side binding: the header declares the four entry
points and PVAC_GATHER_MAX_SOURCES with the ABI version still 3, the library exports them, the ctypes table
of the Python package lists each with the arity of its prototype, and tests/cpp/gather_binding_check.cpp
instantiates the adapter's gather / concat next to the REAL reference headers. CPU only; the compile is
skipped where the reference is absent (the GPU box)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INC = "/root/reference/include"

PROTOS = {
    "pvac_hip_batch_gather_plan": "int pvac_hip_batch_gather_plan(pvac_hip_ctx* ctx, const pvac_gather* G, pvac_ct_batch* dst, "
                                  "uint64_t totals[2]);",
    "pvac_hip_batch_gather_exec": "int pvac_hip_batch_gather_exec(pvac_hip_ctx* ctx, const pvac_gather* G, pvac_ct_batch* dst, "
                                  "uint64_t layer_cap, uint64_t edge_cap);",
    "pvac_hip_batch_gather_path_count": "int pvac_hip_batch_gather_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);",
    "pvac_hip_batch_gather_tile": "int pvac_hip_batch_gather_tile(uint32_t sigma_words, uint32_t out[2]);",
}


def _header():
    with open(os.path.join(ROOT, "include", "pvac_hip.h")) as f:
        return f.read()


def test_header_declares_the_gather_entry_points():
    h = _header()
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    assert re.search(r"#define PVAC_GATHER_MAX_SOURCES 1024\b", h)
    flat = " ".join(h.split())
    for proto in PROTOS.values():
        assert proto in flat, proto
    for field in ("const pvac_ct_batch* srcs;", "uint32_t n_src, pad;", "uint64_t m;", "const uint32_t* pick_src;",
                  "const uint64_t* pick_idx;", "} pvac_gather;"):
        assert field in flat, field
    # the new section follows batch_pack and comes before the PRF
    assert h.index("int pvac_hip_batch_pack(") < h.index("batch_gather\n") < h.index("LPN PRF")


def _lib():
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")
    import pvac_hfhe_cppbyv_amd as pv
    return pv.load_library()


def test_library_exports_them_and_the_abi_is_still_3():
    L = _lib()
    assert L.pvac_hip_abi_version() == 3
    for name in PROTOS:
        assert getattr(L, name).restype is not None


def test_ctypes_table_matches_the_prototypes_arity():
    L = _lib()
    for name, proto in PROTOS.items():
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(",")
        assert len(getattr(L, name).argtypes) == len(params), name


def test_the_gather_structure_has_the_abi_layout():
    import pvac_hfhe_cppbyv_amd as pv
    G = pv.Gather
    assert C.sizeof(G) == 40
    assert [(n, getattr(G, n).offset) for n, _ in G._fields_] == [("srcs", 0), ("n_src", 8), ("pad", 12), ("m", 16),
                                                                  ("pick_src", 24), ("pick_idx", 32)]
    assert pv.GATHER_MAX_SOURCES == 1024


def test_the_tile_geometry_needs_no_context():
    """pvac_hip_batch_gather_tile is host arithmetic: a tile holds at most 16 KiB of edge rows (24 bytes of
    header and weights plus the sigma words) or of 40-byte layer records."""
    L = _lib()
    out = (C.c_uint32 * 2)()
    for sw in (0, 3, 128, 130):
        assert L.pvac_hip_batch_gather_tile(sw, out) == 0
        ept, lpt = out[0], out[1]
        row = 24 + 8 * sw
        assert ept >= 1 and ept * row <= 16384 < (ept + 1) * row
        assert lpt * 40 <= 16384 < (lpt + 1) * 40
    assert L.pvac_hip_batch_gather_tile(0, None) == -22


def test_python_surfaces_exist():
    import pvac_hfhe_cppbyv_amd as pv
    for name in ("gather", "cat", "select", "split", "gather_path_counts"):
        assert callable(getattr(pv.Engine, name))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_INC, "pvac")), reason="reference headers not present")
def test_gather_binding_compiles_against_reference_headers(tmp_path):
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libpvac_hip.so")):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")
    out = str(tmp_path / "gather_binding_check")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-maes", "-mpclmul", "-msse4.1", "-D__HIP_PLATFORM_AMD__", "-I", REF_INC,
           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "gather_binding_check.cpp"), "-o", out, "-pthread",
           "-L", lib, "-lpvac_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert os.path.exists(out)
