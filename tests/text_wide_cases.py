"""The reference-minted fixtures of tests/golden/text_wide (tools/mint_text_wide.cpp): noise plans above
256 pre-merge edges per half. The manifest has the layout of tests/golden/text's; every case is stored
weights-only in parts, and its commits are taken with sigma. TEST INFRASTRUCTURE ONLY."""
import json
import os

import numpy as np

import text_model as tm
from helpers import GOLD, read_ct, splitmix_stream

WIDE = os.path.join(GOLD, "text_wide")


def manifest():
    with open(os.path.join(WIDE, "manifest.json")) as f:
        return json.load(f)


MAN = manifest()
CASES = {c["name"]: c for c in MAN["cases"]}


def case_draws(case):
    if case["log_file"]:
        return np.fromfile(os.path.join(WIDE, case["name"] + ".u64"), dtype=np.uint64)
    return splitmix_stream(case["seed"], 0, case["draws"])


def case_ciphers(case):
    out = []
    for p in range(case["parts"]):
        out += read_ct(os.path.join(WIDE, f"{case['name']}_p{p}.ct"))
    return out


def npre(hint, noise=tm.DEFAULT_NOISE):
    z2, z3 = tm.plan_noise(hint, noise)
    return 8 + 2 * z2 + 3 * z3


def records_equal(got, ref, what):
    assert got.nL == ref.nL and got.nE == ref.nE, what
    for f in ("rule", "ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(got.layers[f], ref.layers[f]), (what, f)
    assert np.array_equal(got.meta, ref.meta), what
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi), what
