"""Regrouping resident batches through the C++ adapter (include/pvac_hip.hpp): tests/cpp/test_gather.cpp,
built by __graft_entry__.build() into tests/cpp/build/test_gather. On the GPU box fixture files go through
Engine::batch_from_image, then Engine::concat / Engine::gather, then Engine::ct_image, and must be the bytes
pvac_ct_write gives for the same regrouping of the host-parsed ciphers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_gather")
GOLD = os.path.join(ROOT, "tests", "golden")
# with sigma: several ciphers, then two files of one
SIGMA = [os.path.join(GOLD, "bounty", "seed3.ct"), os.path.join(GOLD, "bounty", "a.ct"), os.path.join(GOLD, "bounty", "b.ct")]
# weights only: a chain result (10,784 edges), a message of 48 ciphers and one fresh cipher
WEIGHTS = [os.path.join(GOLD, "ref", "chain3.ct"), os.path.join(GOLD, "text", "b1845_p0.ct"), os.path.join(GOLD, "ref", "fr0_x.ct")]


def test_gather_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_gather_adapter():
    assert os.path.exists(EXE), "tests/cpp/build/test_gather missing: build() must compile it"
    # the program itself checks that a group's files agree on sigma nbits and that the mismatched pair does not
    for group in (SIGMA, WEIGHTS):
        for path in group:
            assert os.path.exists(path), path
        r = subprocess.run([EXE] + group, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "checks passed" in r.stdout
    r = subprocess.run([EXE, "--mismatch", SIGMA[1], WEIGHTS[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
