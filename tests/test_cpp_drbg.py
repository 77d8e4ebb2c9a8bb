"""The C++ adapter's device_random forms (include/pvac_hip.hpp): tests/cpp/test_drbg.cpp, built by
__graft_entry__.build() into tests/cpp/build/test_drbg. On the GPU box ct_mul_batch, enc_value_batch and
ct_mul_chain draw every nonce, salt and encryption word from the context's CTR_DRBG and must still decrypt
right, differ between calls, and leave the RandomSource forms' bytes on a replayed stream as they were."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_drbg")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_drbg_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_drbg_adapter():
    assert os.path.exists(EXE), "tests/cpp/build/test_drbg missing: build() must compile it"
    with open(os.path.join(GOLD, "ref", "manifest.json")) as f:
        man = json.load(f)
    with open(os.path.join(GOLD, "ref", "enc_manifest.json")) as f:
        em = json.load(f)
    r = subprocess.run([EXE, GOLD, str(man["canon_tag"]), man["H_digest"], str(em["enc"][0]["v"])], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
