"""pvac_text_pack / pvac_text_unpack (csrc/rt_text.cpp; reference utils/text.hpp:15-37, 63-87): host
memory, no context. Through libpvac_hip.so against the Python restatement in tests/text_model.py, and
as the stand-alone program tests/cpp/test_text_host.cpp built with AddressSanitizer and UBSan
(tests/cpp/Makefile). CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import text_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_text_host")
LENGTHS = [0, 1, 14, 15, 16, 29, 30, 31, 45]


@pytest.fixture(scope="module")
def lib():
    from pvac_hfhe_cppbyv_amd import load_library
    return load_library()


def _msg(n):
    rng = np.random.default_rng(900 + n)
    m = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    if n:
        m[0], m[-1] = 0xFF, 0x00   # a trailing zero byte must survive (the length cipher carries it)
    return bytes(m)


@pytest.mark.parametrize("n", LENGTHS)
def test_pack_unpack_against_restatement(lib, n):
    from pvac_hfhe_cppbyv_amd import text_pack, text_unpack
    msg = _msg(n)
    blocks = text_pack(msg, lib)
    want = tm.text_pack(msg)
    assert len(blocks) == len(want) == -(-n // 15)
    assert [int(lo) | (int(hi) << 64) for lo, hi in blocks] == want
    dec = np.zeros((len(blocks) + 1, 2), np.uint64)
    dec[0, 0] = n
    dec[1:] = blocks
    assert text_unpack(dec, lib) == (msg, 0) == tm.text_unpack([n] + want)


def test_flags_and_capacities(lib):
    from pvac_hfhe_cppbyv_amd import TEXT_LEN_CLIPPED, TEXT_LEN_HI, text_pack, text_unpack
    msg = _msg(31)
    dec = np.zeros((4, 2), np.uint64)
    dec[1:] = text_pack(msg, lib)
    dec[0] = (31, 9)                       # hi != 0: flagged, the low word still counts
    assert text_unpack(dec, lib) == (msg, TEXT_LEN_HI)
    dec[0] = (1000, 0)                     # more than 15 x blocks: clipped, zero padded
    assert text_unpack(dec, lib) == (msg + b"\0" * 14, TEXT_LEN_CLIPPED) == tm.text_unpack([1000] + tm.text_pack(msg))
    dec[0] = (2**64 - 1, 1)
    assert text_unpack(dec, lib)[1] == TEXT_LEN_HI | TEXT_LEN_CLIPPED
    # capacities: PVAC_ENOMEM with the needed size reported, nothing written past the buffer
    n, fl = C.c_size_t(), C.c_uint32()
    dec[0] = (31, 0)
    out = C.create_string_buffer(b"\xAA" * 40, 40)
    assert lib.pvac_text_unpack(C.c_void_p(dec.ctypes.data), 4, out, 30, C.byref(n), C.byref(fl)) == -12 and n.value == 31
    assert out.raw == b"\xAA" * 40
    v = np.full(8, 0xAAAAAAAAAAAAAAAA, np.uint64)
    nb = C.c_size_t()
    assert lib.pvac_text_pack(C.c_char_p(msg), 31, C.c_void_p(v.ctypes.data), 2, C.byref(nb)) == -12 and nb.value == 3
    assert (v == 0xAAAAAAAAAAAAAAAA).all()
    assert lib.pvac_text_pack(C.c_char_p(msg), 31, C.c_void_p(v.ctypes.data), 3, C.byref(nb)) == 0
    assert (v[6:] == 0xAAAAAAAAAAAAAAAA).all()


def test_standalone_program_under_sanitizers():
    """tests/cpp/test_text_host.cpp: its own main over the same helpers, compiled with
    -fsanitize=address,undefined, run as a program."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "build/test_text_host"])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "text host checks passed" in r.stdout
