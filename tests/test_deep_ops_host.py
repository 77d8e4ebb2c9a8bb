"""What ct_lincomb, compact and ct_recrypt accept of a deep cipher, without a GPU (tests/cpp/deep_ops_check.cpp,
built by tests/cpp/deep_ops.mk as a stand-alone host program with ASan + UBSan): the layer bound of a context's
limit, a lincomb term's route at 30,000 / 30,001 / the limit / the limit + 1, the slab of keep / remap words
and its growth, and the classification at the default limit against the rule before the deep-term route."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deep_ops_check(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "deep_ops.mk", "deep_ops_check",
                        f"OUT={tmp_path}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([str(tmp_path / "deep_ops_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "deep_ops_check: ok" in r.stdout
