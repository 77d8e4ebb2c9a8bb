"""The device .ct codec through the C++ adapter (include/pvac_hip.hpp): tests/cpp/test_codec_device.cpp,
built by __graft_entry__.build() into tests/cpp/build/test_codec_device. On the GPU box fixture files
go through Engine::batch_from_image to Engine::ct_image and come back as the same bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_codec_device")
GOLD = os.path.join(ROOT, "tests", "golden")
# with sigma (several ciphers, one cipher), a chain result (hundreds of PROD layers) and weights only
CASES = [os.path.join(GOLD, "bounty", "seed3.ct"), os.path.join(GOLD, "bounty", "a.ct"), os.path.join(GOLD, "ref", "chain3.ct"),
         os.path.join(GOLD, "recrypt", "pool.ct")]


def test_codec_device_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_codec_device_adapter():
    assert os.path.exists(EXE), "tests/cpp/build/test_codec_device missing: build() must compile it"
    for path in CASES:
        assert os.path.exists(path), path
    r = subprocess.run([EXE] + CASES, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
