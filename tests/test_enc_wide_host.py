"""The table logic and host sizing of the wide encryption route without a GPU (tests/cpp/enc_wide_check.cpp,
built by tests/cpp/wide.mk as a stand-alone host program with ASan + UBSan): csrc/enc_wide.hpp's host
instantiation against the brute-force grouping (first occurrences, ranks, stable segments in creation order)
at B = 2, 337 and 65,536, draws_hint, the sub-batch cuts and the scratch layout."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_enc_wide_check(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "wide.mk", "enc_wide_check", f"OUT={tmp_path}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([str(tmp_path / "enc_wide_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "enc_wide_check: ok" in r.stdout
