"""csrc/drbg.hpp, the CTR_DRBG class, without a GPU (tests/cpp/drbg_check.cpp, built by tests/cpp/drbg.mk as
a stand-alone host program): under ASan + UBSan against streams tests/drbg_model.py computes here, and
under ThreadSanitizer with four threads on one instance."""
import os
import subprocess

import numpy as np

import drbg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(target, out):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "drbg.mk", target, f"OUT={out}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _script():
    """instantiate, generate (even, odd, one, zero, beyond a page), reseed, generate_host and device-split
    requests, every output from the model"""
    rng = np.random.default_rng(0xD5B6)
    seed = rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
    g = M.CtrDrbg(seed)
    words = lambda w: w.astype("<u8").tobytes().hex() or "-"
    lines = [f"seed {seed.hex()}"]
    for op, n in [("gen", 5), ("gen", 0), ("dev", 1), ("gen", 4), ("dev", 777), ("gen", 2)]:
        lines.append(f"{op} {n} {words(g.generate(n))}")
    lines.append("counts %d %d %d %d" % g.counts())
    e = rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
    g.reseed(e)
    lines.append(f"reseed {e.hex()}")
    for k in (48, 1, 16, 17):
        lines.append(f"host {k} {g.generate_bytes(k).hex()}")
    lines.append(f"dev 3 {words(g.generate(3))}")
    lines.append("counts %d %d %d %d" % g.counts())
    # a seed whose V ends at 2^128 - 2 cannot be chosen, so the wrap of V + j is covered by drbg_check's
    # own keystream check and by the model's; a second instantiate must forget the first
    seed2 = bytes(48)
    g.seed(seed2)
    lines += [f"seed {seed2.hex()}", f"gen 6 {words(g.generate(6))}", "counts %d %d %d %d" % g.counts()]
    return "\n".join(lines) + "\n"


def test_drbg_check(tmp_path):
    _build("drbg_check", tmp_path)
    script = tmp_path / "script.txt"
    script.write_text(_script())
    r = subprocess.run([str(tmp_path / "drbg_check"), str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "drbg_check: ok" in r.stdout


def test_drbg_check_threads(tmp_path):
    _build("drbg_check_tsan", tmp_path)
    r = subprocess.run([str(tmp_path / "drbg_check_tsan"), "threads"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "drbg_check: ok" in r.stdout
