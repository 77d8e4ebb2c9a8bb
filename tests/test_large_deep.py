"""Host-side planning of deep ct_mul pairs without a GPU (tests/cpp/large_deep_check.cpp, built by
tests/cpp/Makefile as a stand-alone host program with ASan + UBSan): the layer limit of build_large_desc,
a deep pair's scratch layout, and the sub-batch cut that keeps deep and ordinary pairs apart."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_large_deep_check(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "large_deep_check", f"OUT={tmp_path}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([str(tmp_path / "large_deep_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "large_deep_check: ok" in r.stdout
