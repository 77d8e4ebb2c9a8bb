"""The per-context layer limit at the ABI: the header declares the two macros and the three entry
points with the ABI version still 3, the library exports them, load_library() binds each with the
arity of its prototype, and the Python and C++ surfaces exist. CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "pvac_hip_ctx_set_layer_limit": "int pvac_hip_ctx_set_layer_limit(pvac_hip_ctx* ctx, uint32_t max_layers);",
    "pvac_hip_ctx_layer_limit": "int pvac_hip_ctx_layer_limit(pvac_hip_ctx* ctx, uint32_t* out);",
    "pvac_hip_deep_path_count": "int pvac_hip_deep_path_count(pvac_hip_ctx* ctx, uint64_t out[2]);",
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_layer_limit():
    h = _read("include", "pvac_hip.h")
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    assert re.search(r"#define PVAC_LAYER_LIMIT_DEFAULT 16384u\b", h)
    assert re.search(r"#define PVAC_LAYER_LIMIT_MAX \(1u << 24\)", h)
    flat = " ".join(h.split())
    for proto in PROTOS.values():
        assert proto in flat, proto
    # what the limit does not cover is said where it is declared
    assert "ct_lincomb, compact and ct_recrypt" in flat and "30000-layer refusals" in flat


def _lib():
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    assert os.path.exists(lib), "libpvac_hip.so not built (run __graft_entry__.build())"
    import pvac_hfhe_cppbyv_amd as pv
    return pv.load_library()


def test_load_library_binds_them_and_the_abi_is_still_3():
    import ctypes as C
    L = _lib()
    assert L.pvac_hip_abi_version() == 3
    for name, proto in PROTOS.items():
        f = getattr(L, name)
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(",")
        assert f.argtypes is not None and len(f.argtypes) == len(params), name
        assert f.restype is C.c_int, name
    assert L.pvac_hip_ctx_set_layer_limit.argtypes[1] is C.c_uint32
    # null contexts are refused, not dereferenced
    v = C.c_uint32(0)
    assert L.pvac_hip_ctx_set_layer_limit(None, 16384) == -22
    assert L.pvac_hip_ctx_layer_limit(None, C.byref(v)) == -22
    assert L.pvac_hip_deep_path_count(None, (C.c_uint64 * 2)()) == -22


def test_python_and_adapter_surfaces_exist():
    import inspect

    import pvac_hfhe_cppbyv_amd as pv
    assert pv.LAYER_LIMIT_DEFAULT == 16384 and pv.LAYER_LIMIT_MAX == 1 << 24
    assert inspect.signature(pv.Engine.__init__).parameters["layer_limit"].default is None
    assert callable(pv.Engine.set_layer_limit) and callable(pv.Engine.deep_path_counts)
    assert isinstance(pv.Engine.layer_limit, property)
    hpp = " ".join(_read("include", "pvac_hip.hpp").split())
    assert "void set_layer_limit(uint32_t max_layers)" in hpp and "uint32_t layer_limit() const" in hpp
