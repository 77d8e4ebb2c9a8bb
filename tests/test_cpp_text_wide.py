"""enc_text / enc_fp_depth / make_evalkey through the C++ adapter (include/pvac_hip.hpp) above 256 pre-merge
edges per half: tests/cpp/test_text_wide_adapter.cpp, built by __graft_entry__.build() into
tests/cpp/build/test_text_wide_adapter. On the GPU box, with the engine's plan limit raised, pvac_hip::enc_text
replays the 1,875-byte fixture message of tests/golden/text_wide from its logged draws and must give the
fixture's records and every commit with sigma, enc_fp_depth at hint 200 the fpwide fixture, and a recrypt pool
minted at hint 125 ciphers that decrypt to 0."""
import json
import os
import subprocess

import pytest

import text_wide_cases as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_text_wide_adapter")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_text_wide_adapter_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    assert os.path.exists(EXE), "tests/cpp/build/test_text_wide_adapter missing: build() must compile it"
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_text_wide_adapter_against_golden():
    assert os.path.exists(EXE), "tests/cpp/build/test_text_wide_adapter missing: build() must compile it"
    with open(os.path.join(GOLD, "ref", "manifest.json")) as f:
        man = json.load(f)
    c = tw.CASES["b1875"]
    segs = ",".join(f"{x['off']},{x['cnt']}" for x in c["ciphers"])
    commits = ",".join(x["commit"] for x in c["ciphers"])
    text = f"b1875:{c['seed']}:{c['draws']}:0:{c['parts']}:{c['msg_hex']}:{segs}:{commits}"
    f = tw.CASES["fpwide"]
    at = [x["hint"] for x in f["ciphers"]].index(200)
    x = f["ciphers"][at]
    fp = f"{f['seed']}:{f['draws']}:{x['off']}:{x['cnt']}:200:{x['v_lo']}:{x['v_hi']}:{at}:{f['parts']}"
    r = subprocess.run([EXE, GOLD, str(man["canon_tag"]), man["H_digest"], text, fp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
