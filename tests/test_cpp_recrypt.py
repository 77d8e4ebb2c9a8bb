"""ct_recrypt through the C++ adapter (include/pvac_hip.hpp): tests/cpp/test_recrypt.cpp, built by
__graft_entry__.build() into tests/cpp/build/test_recrypt. On the GPU box it replays the draws of the
reference's fixture cases (tests/golden/recrypt) through pvac_hip::ct_recrypt and ct_recrypt_batch and
compares the .ct bytes, checks sigma_density / ubk_apply / compact_edges, and decrypts make_evalkey's
members and a recrypted product."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_recrypt")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_recrypt_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_recrypt_adapter_against_golden():
    assert os.path.exists(EXE), "tests/cpp/build/test_recrypt missing: build() must compile it"
    with open(os.path.join(GOLD, "ref", "manifest.json")) as f:
        man = json.load(f)
    with open(os.path.join(GOLD, "recrypt", "manifest.json")) as f:
        cases = [k for k in json.load(f)["cases"] if k["sigma"]]
    args = [k["name"] + ":" + ",".join(str(d) for d in k["draws"]) for k in cases]
    r = subprocess.run([EXE, GOLD, str(man["canon_tag"]), man["H_digest"]] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
