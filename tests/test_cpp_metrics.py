"""The metrics of utils/metrics.hpp through the C++ adapter (include/pvac_hip.hpp):
tests/cpp/test_metrics.cpp, built by __graft_entry__.build() into tests/cpp/build/test_metrics. On the
GPU box pvac_hip::sigma_shannon / agg_layer_gsum / dump_metrics run on two hand-built ciphers with
sigma: the entropy equals the restated loop bit for bit, the gsums equal the program's own tables, and
dump_metrics appends header then rows to pvac_metrics.csv in a scratch working directory."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_metrics")


def test_metrics_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_metrics_adapter(tmp_path):
    assert os.path.exists(EXE), "tests/cpp/build/test_metrics missing: build() must compile it"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
    with open(tmp_path / "pvac_metrics.csv") as f:
        lines = f.read().splitlines()
    assert lines[0] == "tag,edges,layers,sigma_density,value_lo,value_hi" and len(lines) == 4
