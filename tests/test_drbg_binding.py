"""The device CSPRNG at the ABI: the header declares the six entry points and PVAC_CHAIN_DRBG with the ABI
version still 3, the library exports them, the ctypes table of the Python package binds each with the
arity of its prototype, and the host-only ones answer without a context. CPU only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "pvac_hip_aes256_ctr": "int pvac_hip_aes256_ctr(pvac_hip_ctx* ctx, const uint8_t key[32], const uint8_t ctr_be[16], "
                           "uint64_t* out_dev, size_t n_words);",
    "pvac_hip_drbg_seed": "int pvac_hip_drbg_seed(pvac_hip_ctx* ctx, const uint8_t seed[48]);",
    "pvac_hip_drbg_reseed": "int pvac_hip_drbg_reseed(pvac_hip_ctx* ctx, const uint8_t entropy[48]);",
    "pvac_hip_drbg_fill": "int pvac_hip_drbg_fill(pvac_hip_ctx* ctx, uint64_t* out_dev, size_t n_words);",
    "pvac_hip_drbg_counts": "int pvac_hip_drbg_counts(pvac_hip_ctx* ctx, uint64_t out[4]);",
    "pvac_hip_drbg_tile": "int pvac_hip_drbg_tile(uint32_t out[2]);",
}


def _lib():
    lib = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libpvac_hip.so not built (run __graft_entry__.build())")
    import pvac_hfhe_cppbyv_amd as pv
    return pv.load_library()


def test_header_declares_the_entry_points_and_the_chain_flag():
    with open(os.path.join(ROOT, "include", "pvac_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define PVAC_HIP_ABI_VERSION 3\b", h)
    assert re.search(r"#define PVAC_CHAIN_DRBG 0x800u\b", h)
    flat = " ".join(h.split())
    for proto in PROTOS.values():
        assert proto in flat, proto
    # no existing structure changed: the chain options end where they did
    assert "const pvac_ct_batch* operands; uint32_t n_operands; uint32_t pad3; } pvac_chain_opts;" in flat


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


def test_tile_and_null_contexts_need_no_gpu():
    L = _lib()
    out = (C.c_uint32 * 2)()
    assert L.pvac_hip_drbg_tile(out) == 0
    assert out[0] >= 2 and out[0] % 2 == 0 and 1 <= out[1] <= 65535
    assert L.pvac_hip_drbg_tile(None) == -22
    assert L.pvac_hip_drbg_fill(None, None, 0) == -22
    assert L.pvac_hip_drbg_counts(None, None) == -22


def test_python_surfaces_exist():
    import inspect

    import pvac_hfhe_cppbyv_amd as pv
    for name in ("drbg_seed", "drbg_reseed", "drbg_fill", "aes256_ctr", "drbg_counts", "drbg_tile"):
        assert callable(getattr(pv.Engine, name))
    assert pv.CHAIN_DRBG == 0x800
    assert inspect.signature(pv.Engine.ct_mul).parameters["secure"].default is False
    assert inspect.signature(pv.Engine.ct_mul_chain).parameters["secure"].default is False
    assert inspect.signature(pv.Engine.enc_value).parameters["rnd"].default is None
