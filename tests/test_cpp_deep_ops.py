"""The C++ adapter on deep ciphers (include/pvac_hip.hpp): tests/cpp/test_deep_ops.cpp, built by
__graft_entry__.build() into tests/cpp/build/test_deep_ops. On the GPU box ct_sum, ct_lincomb_batch,
compact_edges and ct_recrypt_batch take ciphers of 30,001 layers on an engine whose limit was raised with
set_layer_limit, deep_route_counts() counts them, and another key's engine at the default limit refuses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_deep_ops")


def test_deep_ops_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_deep_ops_adapter():
    assert os.path.exists(EXE), "tests/cpp/build/test_deep_ops missing: build() must compile it"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
