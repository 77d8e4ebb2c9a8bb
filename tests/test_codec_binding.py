"""The device .ct codec at the ABI: the header declares pvac_ct_index and the pvac_hip_ct_image_* entry
points with the ABI version still 3, the library exports them, and the ctypes table of the Python
package lists each with the arity of its prototype. CPU only."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "pvac_ct_index": "int pvac_ct_index(const uint8_t* buf, size_t len, pvac_ct_file_info* info, uint64_t* pos, size_t pos_cap);",
    "pvac_hip_ct_image_plan": "int pvac_hip_ct_image_plan(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint32_t sigma_bits, "
                              "uint64_t* pos, uint64_t* bytes);",
    "pvac_hip_ct_image_write": "int pvac_hip_ct_image_write(pvac_hip_ctx* ctx, const pvac_ct_batch* X, uint32_t sigma_bits, "
                               "const uint64_t* pos, uint8_t* image, uint64_t cap);",
    "pvac_hip_ct_image_parse": "int pvac_hip_ct_image_parse(pvac_hip_ctx* ctx, const uint8_t* image, uint64_t len, "
                               "const uint64_t* pos, uint64_t n, uint32_t sigma_bits, pvac_ct_batch* X, uint64_t layer_cap, "
                               "uint64_t edge_cap, uint32_t* status);",
    "pvac_hip_ct_image_path_count": "int pvac_hip_ct_image_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);",
}


def _header():
    with open(os.path.join(ROOT, "include", "pvac_hip.h")) as f:
        return f.read()


def test_header_declares_the_codec_entry_points():
    h = _header()
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    flat = " ".join(h.split())
    for proto in PROTOS.values():
        assert proto in flat, proto
    assert ".ct codec (device memory)" in h
    # the new section follows the host codec
    assert h.index(".ct codec (host memory)") < h.index(".ct codec (device memory)")


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


def test_python_surfaces_exist():
    import pvac_hfhe_cppbyv_amd as pv
    from pvac_hfhe_cppbyv_amd import codec
    for name in ("ct_image", "ct_from_image", "ct_image_path_counts"):
        assert callable(getattr(pv.Engine, name))
    for name in ("index", "save_ct_device", "load_ct_device", "load_ct", "save_ct"):
        assert callable(getattr(codec, name))
