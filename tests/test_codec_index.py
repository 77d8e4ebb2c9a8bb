"""pvac_ct_index (csrc/ct_codec.cpp): pvac_ct_scan's validation and sizes plus the byte offset of every
cipher, over every golden .ct file, against the offsets that follow from helpers.read_ct's independent
reader; truncated images, trailing bytes and a pos array that is too small. CPU only."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from helpers import read_ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "**", "*.ct"), recursive=True))
EINVAL, ENOMEM = -22, -12


@pytest.fixture(scope="module")
def codec():
    from pvac_hfhe_cppbyv_amd import codec
    return codec


def _index(codec, buf, cap=None):
    lib = codec._lib()
    a = np.frombuffer(buf, np.uint8)
    info = codec.CtFileInfo()
    pos = np.full(cap if cap is not None else len(buf) // 8 + 2, 0xDEAD, np.uint64)
    rc = lib.pvac_ct_index(C.c_void_p(a.ctypes.data), a.size, C.byref(info), C.c_void_p(pos.ctypes.data), pos.size)
    return rc, info, pos


def _info_tuple(i):
    return (i.n_ciphers, i.total_layers, i.total_edges, i.sigma_bits, i.sigma_words, i.flags)


def test_there_are_fixtures():
    assert len(FILES) >= 40


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.relpath(p, os.path.join(ROOT, "tests", "golden")))
def test_index_matches_scan_and_the_independent_reader(codec, path):
    with open(path, "rb") as f:
        buf = f.read()
    rc, info, pos = _index(codec, buf)
    assert rc == 0
    assert _info_tuple(info) == _info_tuple(codec.scan(buf))
    ciphers = read_ct(path)
    want = [16]
    for c in ciphers:
        layers = sum(9 if int(r) == 1 else 25 for r in c.layers["rule"])
        want.append(want[-1] + 8 + layers + len(c.meta) * (28 + 8 * ((c.nbits + 63) // 64)))
    n = len(ciphers)
    assert info.n_ciphers == n
    assert pos[:n + 1].tolist() == want and want[-1] == len(buf)
    assert (pos[n + 1:] == 0xDEAD).all()
    # the module-level wrapper
    info2, pos2 = codec.index(buf)
    assert pos2.tolist() == want and _info_tuple(info2) == _info_tuple(info)


def test_truncated_and_trailing_bytes_return_scans_codes(codec):
    with open(os.path.join(ROOT, "tests", "golden", "bounty", "seed3.ct"), "rb") as f:
        buf = f.read()
    lib = codec._lib()
    for bad in (buf[:-1], buf[:len(buf) // 2], buf[:15], buf[:16], buf + b"\0", buf + buf[16:], b"\0" * 16 + buf[16:]):
        a = np.frombuffer(bad, np.uint8)
        info = codec.CtFileInfo()
        want = lib.pvac_ct_scan(C.c_void_p(a.ctypes.data), a.size, C.byref(info))
        rc, _, pos = _index(codec, bad)
        assert rc == want == EINVAL
        assert (pos == 0xDEAD).all()


def test_a_pos_array_that_is_too_small_is_enomem(codec):
    with open(os.path.join(ROOT, "tests", "golden", "bounty", "seed3.ct"), "rb") as f:
        buf = f.read()
    n = codec.scan(buf).n_ciphers
    assert n == 9
    rc, info, pos = _index(codec, buf, cap=n)
    assert rc == ENOMEM and info.n_ciphers == n and (pos == 0xDEAD).all()
    rc, info, pos = _index(codec, buf, cap=n + 1)
    assert rc == 0 and pos[0] == 16 and pos[n] == len(buf)


def test_the_empty_file(codec):
    import struct
    buf = struct.pack("<IIQ", 0x66699666, 1, 0)
    rc, info, pos = _index(codec, buf, cap=1)
    assert rc == 0 and info.n_ciphers == 0 and pos[0] == 16
