"""commit_ct through the C++ adapter (include/pvac_hip.hpp): tests/cpp/test_commit.cpp, built by
__graft_entry__.build() into tests/cpp/build/test_commit. On the GPU box pvac_hip::commit_ct and
commit_ct_batch hash the fixture .ct files (one batch mixing ciphers with sigma and weights-only ones)
and must give the digests the reference minted."""
import os
import subprocess

import pytest

from commit_cases import fixture_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_commit")


def test_commit_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_commit_adapter_against_golden():
    assert os.path.exists(EXE), "tests/cpp/build/test_commit missing: build() must compile it"
    man, cases = fixture_cases()
    args = [f"{path}:{int(sig)}:{digest}" for path, sig, digest in cases]
    r = subprocess.run([EXE, str(man["canon_tag"]), man["H_digest"]] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
