"""The Python model of ct_recrypt (tests/recrypt_model.py) pinned to the unmodified reference's
outputs under tests/golden/recrypt/ (minted by tools/mint_recrypt.cpp): byte for byte, iteration
counts and commit_ct digests included. The GPU tests compare the engine with this model."""
import json
import os

import numpy as np
import pytest

import recrypt_model as rm
from helpers import GOLD, REF, Cipher, read_ct

RC = os.path.join(GOLD, "recrypt")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(RC, "manifest.json")) as f:
        man = json.load(f)
    inv = np.fromfile(os.path.join(RC, "ubk_inv.i32"), dtype=np.int32)
    pool = read_ct(os.path.join(RC, "pool.ct"))
    return man, inv, pool


def _layers_view(L):
    """What a .ct file keeps of a layer table: BASE seeds, PROD parents."""
    L = L.copy()
    prod = L["rule"] == 1
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        L[f][prod] = 0
    L["pa"][~prod] = 0
    L["pb"][~prod] = 0
    return L


def test_gen_ubk_matches_the_reference(fx, manifest):
    man, inv, _ = fx
    assert man["canon_tag"] == manifest["canon_tag"]
    perm, got = rm.gen_ubk(manifest["canon_tag"], 8192)
    assert np.array_equal(got, inv)
    assert np.array_equal(np.sort(perm), np.arange(8192)) and np.array_equal(inv[perm], np.arange(8192))


def test_fixture_iteration_counts(fx):
    """The fixtures reach 0, 1, a middle count and 8 iterations, and hold a duplicate-key case."""
    its = {k["name"]: k["iterations"] for k in fx[0]["cases"]}
    assert its["fresh"] == 0 and its["skew_one"] == 1 and 2 <= its["skew_mid"] <= 7 and its["zero_sigma"] == 8
    assert its["doubled"] == 0 and its["product"] == 0
    by = {k["name"]: k for k in fx[0]["cases"]}
    assert by["doubled"]["in_edges"] == 2 * by["doubled"]["out_edges"]
    assert fx[0]["pool"] == 4 and len(fx[2]) == 4


def test_model_reproduces_every_fixture(oracle, manifest, fx):
    man, inv, pool = fx
    Hd = bytes.fromhex(manifest["H_digest"])
    for k in man["cases"]:
        src = os.path.join(RC, k["name"] + "_in.ct") if k["sigma"] else os.path.join(REF, "pair0_mul.ct")
        x = read_ct(src)[0]
        assert x.nE == k["in_edges"] and x.nL == k["in_layers"]
        draws = list(k["draws"]) + [0] * (8 - len(k["draws"]))
        got, it = rm.recrypt(oracle, x, pool, draws, inv)
        ref = read_ct(os.path.join(RC, k["name"] + "_out.ct"))[0]
        assert it == k["iterations"] == len(k["draws"]), k["name"]
        L = _layers_view(got.layers)
        for f in ("rule", "pa", "pb", "ztag", "nonce_lo", "nonce_hi"):
            assert np.array_equal(L[f], ref.layers[f]), (k["name"], f)
        assert np.array_equal(got.meta, ref.meta), k["name"]
        assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi), k["name"]
        if k["sigma"]:
            assert np.array_equal(got.sigma, ref.sigma), k["name"]
        assert oracle.commit(got, manifest["canon_tag"], Hd).hex() == k["commit"], k["name"]


def test_doubled_cipher_merges_to_zero_sigmas(fx):
    x = read_ct(os.path.join(RC, "doubled_in.ct"))[0]
    out = read_ct(os.path.join(RC, "doubled_out.ct"))[0]
    assert out.nE * 2 == x.nE and not out.sigma.any()


@pytest.mark.parametrize("ones,iterates", [(101376, False), (101375, True), (103424, False), (103425, True)])
def test_density_thresholds_are_strict(ones, iterates):
    """25 edges of 8192 bits: 101,376 ones are exactly 0.495 and 103,424 exactly 0.505; the reference
    iterates only for d < 0.495 or d > 0.505 (recrypt.hpp:21-24)."""
    assert rm.needs_balance(ones, 25, 8192) == iterates


def test_apply_perm_and_popcount():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 2**64, (3, 128), dtype=np.uint64)
    inv = rng.permutation(8192).astype(np.int32)
    t = rm.apply_perm(s, inv, 8192)
    assert rm.popcount(t) == rm.popcount(s)
    for src in (0, 63, 64, 8191, 4097):
        j = int(inv[src])
        assert ((t[:, j // 64] >> np.uint64(j % 64)) & np.uint64(1)).tolist() == \
            ((s[:, src // 64] >> np.uint64(src % 64)) & np.uint64(1)).tolist()
    back = np.zeros(8192, np.int32)
    back[inv] = np.arange(8192, dtype=np.int32)
    assert np.array_equal(rm.apply_perm(t, back, 8192), s)
