"""The CPU model of the gsum checker (gsum_model.py) pinned without a GPU: it holds on the reference's
own ct_mul outputs and on the pinned port's, its exact sums agree with the reference's literal
fp_add / fp_sub chains, and every mutation that test_gpu_check.py gives the kernel is classified
here as the table says, so those inputs really separate a right checker from a wrong one."""
import json
import os

import numpy as np
import pytest

import gsum_cases as gc
from gsum_model import EDGE_LIMIT, layer_gsums, layer_gsums_chain, status, status_chain
from helpers import REF, Cipher, P, pack_meta, read_ct, read_layers_u64, read_u64

CHAIN_EDGES = 4000   # status_chain costs one oracle call per edge: compared up to this many


def _both(oracle, t, powg, Bm):
    s = status(oracle, t.A, t.B, t.C, t.nz, powg, Bm)
    if t.A.nE + t.B.nE + t.C.nE <= CHAIN_EDGES:
        assert status_chain(oracle, t.A, t.B, t.C, t.nz, powg, Bm) == s, t.name
    return s


def _fixture_triples():
    with open(os.path.join(REF, "fr_manifest.json")) as f:
        nfr = len(json.load(f)["cases"])
    for stem in [f"pair{p}" for p in range(8)] + [f"fr{k}" for k in range(nfr)]:
        x, y = (read_ct(os.path.join(REF, f"{stem}_{s}.ct"))[0] for s in "xy")
        w = read_ct(os.path.join(REF, f"{stem}_mul_w.ct"))[0]
        C = Cipher(read_layers_u64(f"{stem}_mul_layers.u64"), w.meta, w.w_lo, w.w_hi)   # .ct drops PROD nonces
        yield gc.Triple(x, y, C, read_u64(f"{stem}_mul_stream.u64")[:2 * x.nL * y.nL], stem)
    x, y = (read_ct(os.path.join(REF, f"pair0_{s}.ct"))[0] for s in "xy")
    w = read_ct(os.path.join(REF, "pair0_mul.ct"))[0]       # the WITH_SIGMA product
    yield gc.Triple(x, y, Cipher(read_layers_u64("pair0_mul_layers.u64"), w.meta, w.w_lo, w.w_hi),
                    read_u64("pair0_mul_stream.u64")[:2 * x.nL * y.nL], "pair0 sigma")


def test_model_holds_on_reference_products(oracle):
    """The reference's own ct_mul outputs (the fixtures of test_ct_mul_weights_golden_batched,
    test_ct_mul_sigma_golden and the full-range cases) with the recorded nonces and the key's powg_B."""
    powg = read_u64("powg_B.u64")
    n = 0
    for t in _fixture_triples():
        assert t.C.nE > 0
        assert _both(oracle, t, powg, 337) == 0, t.name
        n += 1
    assert n >= 10


@pytest.mark.parametrize("Bm", [337, 1022])
def test_model_holds_on_oracle_products(oracle, Bm):
    """ct_mul of random multi-layer inputs, special and non-canonical weights on both sides, idx over
    the whole range and narrow (sums wrap mod B)."""
    rng = np.random.default_rng([0x70, Bm])
    powg = gc.key_powg(Bm)
    for la, lb, span in ((1, 1, Bm), (2, 2, Bm), (3, 2, 24), (2, 5, 3), (4, 1, Bm)):
        A = gc.rand_cipher(rng, la, Bm, idx_span=span, special=True)
        B = gc.rand_cipher(rng, lb, Bm, idx_span=span, special=True)
        nz = rng.integers(0, 2**64, (la * lb, 2), dtype=np.uint64)
        t = gc.Triple(A, B, oracle.ct_mul(A, B, nz.reshape(-1), Bm=Bm), nz, f"{la}x{lb}")
        assert _both(oracle, t, powg, Bm) == 0, t.name
        # and the sums themselves: the chain's words are the exact residues
        for X in (t.A, t.B, t.C):
            assert [lo | hi << 64 for lo, hi in layer_gsums_chain(oracle, X, powg)] == layer_gsums(oracle, X, powg)


def test_gsum_is_the_plain_sum(oracle):
    """layer_gsums against a direct Python restatement (no oracle): sum of +/- w g^idx mod p."""
    rng = np.random.default_rng(0x71)
    powg = gc.key_powg(337)
    pg = gc.powg_int(powg)
    X = gc.rand_cipher(rng, 3, 337, special=True)
    X.meta[0] = pack_meta(7, 5, 1)      # names no layer: ignored
    want = [0, 0, 0]
    for e in range(1, X.nE):
        t = ((int(X.w_hi[e]) << 64 | int(X.w_lo[e])) % P) * pg[int(X.idx()[e])]
        want[int(X.layer_id()[e])] += t if X.ch()[e] == 0 else -t
    assert layer_gsums(oracle, X, powg) == [v % P for v in want]


@pytest.mark.parametrize("mode", ["lds", "slab"])
@pytest.mark.parametrize("Bm", [337, 1022])
def test_mutation_table_is_classified_as_listed(oracle, Bm, mode):
    """Every base holds; every mutation of a plain base gives the status its row lists (1 rows do not
    land on a zero product by accident, 0 rows are not stricter than the reference); every row
    occurs; exact sums and literal chains agree on every case."""
    powg = gc.key_powg(Bm)
    seen, ones = set(), 0
    for name, t, want in gc.cases(oracle, Bm, mode):
        s = _both(oracle, t, powg, Bm)
        if want is not None:
            assert s == want, (t.name, s, want)
            seen.add(name)
        elif t.plain:
            seen.add(name)
        ones += s == 1
    assert seen >= set(gc.ROWS), set(gc.ROWS) - seen
    assert ones > 40
    if mode == "slab":
        for name, t, _ in gc.cases(oracle, Bm, mode):
            assert gc.table_bytes(Bm, t.A.nL, t.B.nL, t.C.nL, t.A.nL * t.B.nL) > gc.LDS_BUDGET, t.name
    else:
        mx = lambda f: max(f(t) for _, t, _ in gc.cases(oracle, Bm, mode))
        assert gc.table_bytes(Bm, mx(lambda t: t.A.nL), mx(lambda t: t.B.nL), mx(lambda t: t.C.nL),
                              mx(lambda t: t.A.nL * t.B.nL)) <= gc.LDS_BUDGET


def test_status_precedence_and_edge_limit(oracle):
    """3 (a cipher of 2^21 edges or more) before 2 (idx >= B) before the invariant; 2^21 - 1 edges are
    still checked. Counts only: the model looks at no weight before it returns 3."""
    rng = np.random.default_rng(0x72)
    powg = gc.key_powg(337)
    t = gc.product_triple(oracle, rng, 1, 1, 337, "1x1")
    t.C.w_lo[0] ^= np.uint64(1)
    assert status(oracle, t.A, t.B, t.C, t.nz, powg, 337) == 1
    t.B.meta[0] = pack_meta(0, 337, 0)
    assert status(oracle, t.A, t.B, t.C, t.nz, powg, 337) == 2
    z = np.zeros(EDGE_LIMIT, np.uint64)
    big = Cipher(t.A.layers, z, z, z)
    assert status(oracle, big, t.B, t.C, t.nz, powg, 337) == 3
    assert status(oracle, t.A, t.B, big, t.nz, powg, 337) == 3
    t.B.meta[0] = pack_meta(0, 336, 0)
    almost = Cipher(t.A.layers, z[1:], z[1:], z[1:])      # 2^21 - 1 zero weights: gsum 0
    assert status(oracle, almost, t.B, Cipher(t.C.layers, z[:0], z[:0], z[:0]), t.nz, powg, 337) == 0
