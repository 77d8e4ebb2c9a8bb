"""The ct_lincomb model (tests/lincomb_model.py) against itself and against the reference: the fold
through the oracle's ct_add equals "compact every term, then concatenate" on a seeded mixed batch at
every prefix length, and the fold reproduces every commit_ct of tests/golden/lincomb/manifest.json
(minted by tools/mint_lincomb.cpp with the unmodified reference). CPU only."""
import numpy as np
import pytest

import lincomb_model as lm
from helpers import LAYER_DT, Cipher, pack_meta


def synthetic(rng, n_layers, n_edges, unused=(), prod=()):
    """A cipher of n_layers layers inside the contract: `prod` = (layer, pa, pb) PROD records, no edge
    points at a layer of `unused`; weights anywhere in [0, 2^128)."""
    layers = np.zeros(n_layers, LAYER_DT)
    layers["ztag"] = rng.integers(0, 2**63, n_layers, dtype=np.uint64)
    layers["nonce_lo"] = rng.integers(0, 2**63, n_layers, dtype=np.uint64)
    layers["nonce_hi"] = rng.integers(0, 2**63, n_layers, dtype=np.uint64)
    for l, pa, pb in prod:
        layers[l] = (1, pa, pb, 0, 0, 0, 0)
    ok = np.array([l for l in range(n_layers) if l not in set(unused)], np.uint64)
    lid = ok[rng.integers(0, len(ok), n_edges)] if len(ok) else np.zeros(0, np.uint64)
    n_edges = len(lid)
    meta = pack_meta(lid, rng.integers(0, 337, n_edges), rng.integers(0, 2, n_edges))
    return Cipher(layers, meta, rng.integers(0, 2**64, n_edges, dtype=np.uint64),
                  rng.integers(0, 2**64, n_edges, dtype=np.uint64))


def mixed_pool():
    rng = np.random.default_rng(0x11C0)
    g = lm.golden_cipher
    pool = [lm.strip(g(p)) for p in ("ref/enc0.ct", "ref/enc1.ct", "lincomb/unused_in.ct", "ref/pair0_mul_w.ct",
                                     "ref/chain1.ct", "ref/fr0_x.ct", "ref/fr1_x.ct")]
    pool.append(lm.empty_cipher())
    # an unused BASE layer (1), and an unused PROD layer (4) whose parents (2, 3) nothing else uses
    pool.append(synthetic(rng, 6, 30, unused=(1, 2, 3, 4), prod=((4, 2, 3),)))
    # a used PROD layer (3) that keeps its otherwise unused parents (0, 5) alive; 1 is dropped
    pool.append(synthetic(rng, 6, 25, unused=(0, 1, 5), prod=((3, 0, 5),)))
    return pool


def test_fold_equals_compact_then_concat(oracle):
    pool = mixed_pool()
    rng = np.random.default_rng(7)
    term = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), 6)])   # every cipher, then repeats
    scales = [int(x) for x in (0, 1, lm.P - 1, lm.P, 2**128 - 1, 5, 2**64 + 3)] * 3
    scales = scales[:len(term)]
    flags = rng.integers(0, 2, len(term)).astype(np.uint32)
    for m in range(len(term) + 1):
        a = lm.fold(oracle, pool, term[:m], scales[:m], flags[:m])
        b = lm.concat(oracle, pool, term[:m], scales[:m], flags[:m])
        assert lm.same(a, b), m
    # unscaled (scale = None) and all-scaled (flags = None) forms
    assert lm.same(lm.fold(oracle, pool, term), lm.concat(oracle, pool, term))
    assert lm.same(lm.fold(oracle, pool, term, scales), lm.concat(oracle, pool, term, scales))


def test_unscaled_terms_keep_raw_words(oracle):
    """fp_mul by 1 canonicalises a non-canonical weight, so "unscaled" is not "scaled by 1"."""
    x = lm.strip(lm.golden_cipher("ref/fr0_x.ct"))
    raw = lm.fold(oracle, [x], [0])
    one = lm.fold(oracle, [x], [0], [1])
    assert np.array_equal(raw.w_lo, x.w_lo) and np.array_equal(raw.w_hi, x.w_hi)
    assert not (np.array_equal(one.w_lo, x.w_lo) and np.array_equal(one.w_hi, x.w_hi))


@pytest.mark.parametrize("name", [c["name"] for c in lm.manifest()["cases"]])
def test_fold_reproduces_reference_commit(oracle, name):
    man = lm.manifest()
    case = next(c for c in man["cases"] if c["name"] == name)
    pool, term, scales, flags = lm.case_inputs(case)
    out = lm.fold(oracle, pool, term, scales, flags, edge_budget=case["edge_budget"], sigma=case["sigma"])
    assert (out.nL, out.nE) == (case["out_layers"], case["out_edges"])
    assert oracle.commit(out, man["canon_tag"], bytes.fromhex(man["H_digest"])).hex() == case["commit"]
