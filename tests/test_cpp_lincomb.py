"""ct_sum / ct_lincomb / ct_lincomb_batch through the C++ adapter (include/pvac_hip.hpp):
tests/cpp/test_lincomb.cpp, built by __graft_entry__.build() into tests/cpp/build/test_lincomb. On the
GPU box it runs every case of tests/golden/lincomb/manifest.json and must commit to the digests the
reference minted; the cases of one edge budget share a run (one engine per public key)."""
import os
import subprocess

import pytest

import lincomb_model as lm
from helpers import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_lincomb")


def test_lincomb_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    if not os.path.exists(EXE):
        pytest.skip("tests/cpp not built (run __graft_entry__.build())")
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
@pytest.mark.parametrize("budget", sorted({c["edge_budget"] for c in lm.manifest()["cases"]}))
def test_lincomb_adapter_against_golden(tmp_path, budget):
    assert os.path.exists(EXE), "tests/cpp/build/test_lincomb missing: build() must compile it"
    man = lm.manifest()
    lines = []
    for c in man["cases"]:
        if c["edge_budget"] != budget:
            continue
        lines.append(f"{c['name']} {int(c['sigma'])} {c['commit']} {len(c['terms'])}")
        lines += [f"{p} {f} {s[0]} {s[1]}" for p, f, s in zip(c["terms"], c["flags"], c["scales"])]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    r = subprocess.run([EXE, str(man["canon_tag"]), man["H_digest"], str(budget), GOLD, str(cases)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
