"""The per-context encryption plan limit at the ABI: the header declares the macros, the flag and the five
entry points with the ABI version still 3, the library exports them, load_library() binds each with the arity
of its prototype, null contexts are refused, and the Python and C++ surfaces exist. What needs a context (the
limit's default, range and getter, the sizes at hint 125, the refusal above a raised limit) is in
test_gpu_text_wide.py::test_defaults_and_refusals; the sub-batch cuts and draws_hint are checked on the CPU
by test_enc_wide_host.py. CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "pvac_hip_ctx_set_enc_plan_limit": "int pvac_hip_ctx_set_enc_plan_limit(pvac_hip_ctx* ctx, uint32_t max_pre_edges);",
    "pvac_hip_ctx_enc_plan_limit": "int pvac_hip_ctx_enc_plan_limit(pvac_hip_ctx* ctx, uint32_t* out);",
    "pvac_hip_ctx_set_enc_budget": "int pvac_hip_ctx_set_enc_budget(pvac_hip_ctx* ctx, uint64_t pre_edges);",
    "pvac_hip_ctx_enc_budget": "int pvac_hip_ctx_enc_budget(pvac_hip_ctx* ctx, uint64_t* out);",
    "pvac_hip_enc_path_count": "int pvac_hip_enc_path_count(pvac_hip_ctx* ctx, uint64_t out[4]);",
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_plan_limit():
    h = _read("include", "pvac_hip.h")
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    assert re.search(r"#define PVAC_ENC_PLAN_LIMIT_DEFAULT 256u\b", h)
    assert re.search(r"#define PVAC_ENC_PLAN_LIMIT_MAX \(1u << 24\)", h)
    assert re.search(r"#define PVAC_ENC_BUDGET_DEFAULT \(1ull << 22\)", h)
    assert re.search(r"#define PVAC_ENC_WITH_SIGMA 0x1u\b", h) and re.search(r"#define PVAC_ENC_WIDE_ALL 0x2u\b", h)
    flat = " ".join(h.split())
    for proto in PROTOS.values():
        assert proto in flat, proto
    # why the default stays is said where it is declared
    doc = " ".join(h.replace("*", " ").split())   # comment text without its line markers
    assert "about 1 KB per pre-merge edge" in doc and "square of its length" in doc


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
    assert L.pvac_hip_ctx_set_enc_plan_limit.argtypes[1] is C.c_uint32
    assert L.pvac_hip_ctx_set_enc_budget.argtypes[1] is C.c_uint64
    # null contexts are refused, not dereferenced
    v, w = C.c_uint32(0), C.c_uint64(0)
    assert L.pvac_hip_ctx_set_enc_plan_limit(None, 256) == -22
    assert L.pvac_hip_ctx_enc_plan_limit(None, C.byref(v)) == -22
    assert L.pvac_hip_ctx_set_enc_budget(None, 1) == -22
    assert L.pvac_hip_ctx_enc_budget(None, C.byref(w)) == -22
    assert L.pvac_hip_enc_path_count(None, (C.c_uint64 * 4)()) == -22


def test_python_and_adapter_surfaces_exist():
    import inspect

    import pvac_hfhe_cppbyv_amd as pv
    assert pv.ENC_PLAN_LIMIT_DEFAULT == 256 and pv.ENC_PLAN_LIMIT_MAX == 1 << 24 and pv.ENC_BUDGET_DEFAULT == 1 << 22
    assert pv.ENC_WIDE_ALL == 2
    assert inspect.signature(pv.Engine.__init__).parameters["enc_plan_limit"].default is None
    assert inspect.signature(pv.Engine.enc_items).parameters["wide_all"].default is False
    assert callable(pv.Engine.set_enc_plan_limit) and callable(pv.Engine.set_enc_budget) and callable(pv.Engine.enc_path_counts)
    assert isinstance(pv.Engine.enc_plan_limit, property) and isinstance(pv.Engine.enc_budget, property)
    hpp = " ".join(_read("include", "pvac_hip.hpp").split())
    assert "void set_enc_plan_limit(uint32_t max_pre_edges)" in hpp and "uint32_t enc_plan_limit() const" in hpp
    assert "engine_for(pk).set_enc_plan_limit(n)" in hpp
