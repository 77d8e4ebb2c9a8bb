"""enc_text / dec_text / enc_fp_depth through the C++ adapter (include/pvac_hip.hpp):
tests/cpp/test_text_adapter.cpp, built by __graft_entry__.build() into tests/cpp/build/test_text_adapter.
On the GPU box pvac_hip::enc_text replays every fixture message of tests/golden/text from a source
that serves each cipher's logged segment padded to the words the adapter takes, and must give the
files' bytes; pvac_hip::dec_text returns the messages; all messages again as one batch. What the adapter
wrote is then decrypted without the engine: by the CPU oracle's dec_value and the restated unpack, and by
the reference's own dec_text where its tool was built (oracle/_ref/mint_text, tools/mint_text.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

import text_model as tm
from helpers import Cipher, fixture_secret, read_ct, read_u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_text_adapter")
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["empty", "one", "b15", "b16", "b30", "b31", "utf8", "b240", "b1845"]


def test_text_adapter_binary_links():
    """CPU-side: the test program was built and resolves libpvac_hip.so in-tree."""
    assert os.path.exists(EXE), "tests/cpp/build/test_text_adapter missing: build() must compile it"
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if "libpvac_hip.so" in l]
    assert line and "not found" not in line[0]
    assert os.path.join("pvac_hfhe_cppbyv_amd", "lib") in os.path.normpath(line[0].split("=>")[1])


@pytest.mark.gpu
def test_text_adapter_against_golden(oracle, tmp_path):
    assert os.path.exists(EXE), "tests/cpp/build/test_text_adapter missing: build() must compile it"
    with open(os.path.join(GOLD, "ref", "manifest.json")) as f:
        man = json.load(f)
    cases = {c["name"]: c for c in tm.manifest()["cases"]}
    args = []
    for n in NAMES:
        c = cases[n]
        segs = ",".join(f"{x['off']},{x['cnt']}" for x in c["ciphers"])
        args.append(f"{n}:{c['seed']}:{c['draws']}:{int(c['sigma'])}:{c['parts']}:{c['msg_hex'] or '-'}:{segs}")
    r = subprocess.run([EXE, GOLD, str(man["canon_tag"]), man["H_digest"]] + args, capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, PVAC_TEXT_DUMP=str(tmp_path)))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
    # the adapter's output decrypted off the engine
    sk, _, _ = fixture_secret()
    powg = read_u64("powg_B.u64")
    ref_tool = os.path.join(ROOT, "oracle", "_ref", "mint_text")
    for n in NAMES:
        msg = bytes.fromhex(cases[n]["msg_hex"])
        path = os.path.join(str(tmp_path), n + ".ct")
        if n != "b1845":   # a CPU PRF evaluation per cipher: the 124-cipher message is left to the reference's tool
            vals = []
            for c in read_ct(path):
                R = np.zeros(2 * c.nL, np.uint64)
                for i, L in enumerate(c.layers):
                    R[2 * i:2 * i + 2] = oracle.prf_R(sk, man["canon_tag"], (int(L["ztag"]), int(L["nonce_lo"]), int(L["nonce_hi"])))
                lo, hi = oracle.dec(Cipher(c.layers, c.meta, c.w_lo, c.w_hi), powg, R)
                vals.append(lo | (hi << 64))
            assert tm.text_unpack(vals) == (msg, 0), n
        if os.path.exists(ref_tool) and n in ("b31", "utf8", "b1845"):
            d = subprocess.run([ref_tool, os.path.join(GOLD, "ref"), "--dec", path], capture_output=True, text=True, timeout=120)
            assert d.returncode == 0 and f"dec_text {msg.hex()}\n" in d.stdout, (n, d.stdout[-200:], d.stderr[-200:])
