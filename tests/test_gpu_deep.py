"""GPU parity of deep ciphers (k_large_deep.hip): ct_mul pairs of more than 16,384 layers before
compaction and ct_add / ct_sub pairs of more than 30,000, accepted under a raised per-context layer limit
(Engine(layer_limit=...)). Every output cipher is compared in full with the pinned CPU oracle: layers with
remapped parents and ztags, meta, both weight words, and sigma where it is asked for. B = 7 keeps the key
space |A.L||B.L|B (and the scratch, ~16 words per key slot) small; one case runs at B = 337."""
import ctypes as C

import numpy as np
import pytest

from helpers import LAYER_DT, Cipher, default_params, pack_device_batch, splitmix_stream

pytestmark = pytest.mark.gpu

B7 = 7
LIMIT = 1 << 20


def _dev_batch(eng, ciphers, sigma=False):
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    hc = [HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in ciphers]
    return DeviceBatch.from_host(hc, eng.device, sigma=sigma)


def _i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64))


def _same(got, ref, sigma=False):
    for f in ("rule", "pa", "pb", "ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(got.layers[f], ref.layers[f]), f
    assert got.nE == ref.nE
    assert np.array_equal(got.meta, ref.meta)
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi)
    if sigma:
        assert got.sigma is not None and np.array_equal(got.sigma, ref.sigma)


def _base_layers(rng, nl):
    L = np.zeros(nl, LAYER_DT)
    L["ztag"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    L["nonce_lo"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    L["nonce_hi"] = rng.integers(0, 2**63, nl, dtype=np.uint64)
    return L


def _meta(lay, idx, ch):
    return (np.asarray(lay, np.uint64) | (np.asarray(idx, np.uint64) << np.uint64(32))
            | (np.asarray(ch, np.uint64) << np.uint64(48)))


def _mk(rng, nl, ne, B=B7, at=(), full=False, layers=None):
    """nl BASE layers (or `layers`), ne edges on random layers plus one on each layer of `at`; full: weights
    over all of 2^128 (non-canonical words included), else below 2^126."""
    lay = np.concatenate([np.asarray(at, np.uint64), rng.integers(0, nl, ne).astype(np.uint64)])
    n = len(lay)
    rng.shuffle(lay)
    idx = rng.integers(0, B, n).astype(np.uint64)
    ch = rng.integers(0, 2, n).astype(np.uint64)
    top = 2**64 - 1 if full else 2**62
    lo = rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    hi = rng.integers(0, top, n, dtype=np.uint64, endpoint=True)
    return Cipher(_base_layers(rng, nl) if layers is None else layers, _meta(lay, idx, ch), lo, hi)


def _run_mul(eng, xs, ys, seed, flags=0, with_salts=False):
    """Batched ct_mul_plan / ct_mul with random nonces (and salts): host outputs, the plan, each pair's
    product nonces, the device batches and nonces for a second run, the salts."""
    A, Bb = _dev_batch(eng, xs), _dev_batch(eng, ys)
    Cb, plan = eng.ct_mul_plan(A, Bb)
    loff = Cb.l_off.cpu().numpy().view(np.uint64)
    eoff = Cb.e_off.cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(seed)
    nonces = rng.integers(0, 2**63, 2 * max(plan.total_layer_slots, 1), dtype=np.uint64)
    salts = rng.integers(0, 2**63, max(plan.total_edge_slots, 1), dtype=np.uint64)
    per = []
    for p, (x, y) in enumerate(zip(xs, ys)):
        base = int(loff[p]) + x.nL + y.nL
        per.append(nonces[2 * base:2 * base + 2 * x.nL * y.nL].copy())
    dn = _i64(nonces).to(eng.device)
    kw = {"salts": _i64(salts).to(eng.device)} if with_salts else {}
    out = eng.ct_mul(A, Bb, nonces=dn, C_=Cb, plan=plan, flags=flags, **kw)
    return out.to_host(), plan, per, (A, Bb, out, dn), (salts, eoff)


def _check_pairs(oracle, out, xs, ys, per, canon_tag=0, edge_budget=1200000, B=B7, skip=()):
    for p, (x, y) in enumerate(zip(xs, ys)):
        if p in skip:
            continue
        _same(out[p], oracle.ct_mul(x, y, per[p], canon_tag=canon_tag, edge_budget=edge_budget, Bm=B))


def _engine(**kw):
    from pvac_hfhe_cppbyv_amd import Engine
    kw.setdefault("B", B7)
    kw.setdefault("layer_limit", LIMIT)
    return Engine(device=0, **kw)


# ------------------------------------------------------------------ 1. boundary
def test_boundary_16384_and_16385(oracle):
    """One batch: (4, 3276) plans exactly 16,384 layers (the existing kernels), (1, 8192) and (8192, 1) plan
    16,385 (the deep kernels). All bit-exact, two deep pairs counted, every status 0."""
    rng = np.random.default_rng(0xDE01)
    xs = [_mk(rng, 4, 40), _mk(rng, 1, 6), _mk(rng, 8192, 40, at=(0, 8191))]
    ys = [_mk(rng, 3276, 40, at=(0, 3275)), _mk(rng, 8192, 40, at=(0, 8191)), _mk(rng, 1, 6)]
    assert [x.nL + y.nL + x.nL * y.nL for x, y in zip(xs, ys)] == [16384, 16385, 16385]
    eng = _engine(canon_tag=0xDE)
    assert eng.layer_limit == LIMIT and eng.deep_path_counts() == (0, 0)
    out, plan, per, _, _ = _run_mul(eng, xs, ys, 1)
    assert plan.n_large == 3
    assert eng.deep_path_counts() == (2, 0)
    assert list(eng.ct_mul_status(3)) == [0, 0, 0]
    _check_pairs(oracle, out, xs, ys, per, canon_tag=0xDE)


# ------------------------------------------------------------------ 2. wide layer ids
def test_wide_layer_ids(oracle):
    """(33000, 1), (70000, 1) and (1, 70000): edges on layers 0, 32767, 32768, 65535, 65536 and the last one
    among random ones: ids beyond 15 and 16 bits on either side (at 2^16 A layers the pair takes one
    products workgroup per task)."""
    rng = np.random.default_rng(0xDE02)
    marks = lambda nl: [l for l in (0, 32767, 32768, 65535, 65536, nl - 1) if l < nl]
    xs = [_mk(rng, 33000, 120, at=marks(33000)), _mk(rng, 70000, 120, at=marks(70000)), _mk(rng, 1, 5)]
    ys = [_mk(rng, 1, 5), _mk(rng, 1, 5), _mk(rng, 70000, 120, at=marks(70000))]
    eng = _engine(canon_tag=0xDF)
    out, plan, per, _, _ = _run_mul(eng, xs, ys, 2)
    assert eng.deep_path_counts()[0] == 3 and list(eng.ct_mul_status(3)) == [0, 0, 0]
    _check_pairs(oracle, out, xs, ys, per, canon_tag=0xDF)
    # the marked layers carry edges in the output (compacted ids, so by their seeds)
    for p, big in ((0, xs[0]), (1, xs[1]), (2, ys[2])):
        kept = set(out[p].layers["nonce_lo"][out[p].layers["rule"] == 0].tolist())
        for l in marks(big.nL):
            assert int(big.layers["nonce_lo"][l]) in kept


# ------------------------------------------------------------------ 3. dense square
@pytest.mark.parametrize("B,ne", [(7, 400), (337, 60)])
def test_dense_square(oracle, B, ne):
    """(128, 128), Lc = 16,640: duplicates of (layer, idx, ch), both channels, weights over all of 2^128
    (non-canonical words included); 400 edges a side at B = 7, 60 a side at B = 337."""
    rng = np.random.default_rng(0xDE03 + B)
    x, y = _mk(rng, 128, ne, B=B, full=True), _mk(rng, 128, ne, B=B, full=True)
    if B == 7:   # 400 edges over 128 x 14 cells: duplicates are certain, and stated
        assert len(np.unique(x.meta)) < x.nE and set(x.ch().tolist()) == {0, 1}
    eng = _engine(B=B, canon_tag=0xE0)
    out, plan, per, _, _ = _run_mul(eng, [x], [y], 3)
    assert eng.deep_path_counts()[0] == 1 and list(eng.ct_mul_status(1)) == [0]
    _check_pairs(oracle, out, [x], [y], per, canon_tag=0xE0, B=B)


# ------------------------------------------------------------------ 4. closure
def _closure_cipher(rng, nl=6000):
    """BASE layers below 3000, PROD layers above with parents anywhere below them (chains many levels
    deep), three PROD layers whose parents have LARGER indices, edges only on a few high layers and a
    few BASE ones: most BASE layers stay unused."""
    L = _base_layers(rng, nl)
    for l in range(3000, nl):
        L[l] = (1, int(rng.integers(0, l)), int(rng.integers(0, l)), 0, 0, 0, 0)
    # depth >= 3 by construction: 5999 -> 5998 -> 5997 -> 5996 (a BASE parent beside each)
    for l in (5999, 5998, 5997):
        L[l]["pa"], L[l]["pb"] = l - 1, int(rng.integers(0, 3000))
    # parents above their child: 20 -> 5500 -> 21 -> 5400: one ascending sweep cannot close this
    L[20] = (1, 5500, 7, 0, 0, 0, 0)
    L[5500]["pa"], L[5500]["pb"] = 21, 8
    L[21] = (1, 5400, 9, 0, 0, 0, 0)
    at = [5999, 20] + rng.integers(5000, nl, 30).tolist() + rng.integers(0, 3000, 30).tolist()
    return _mk(rng, nl, 0, at=at, layers=L)


def test_closure_fixed_point_and_identity(oracle):
    """compact_layers over a deep pair: PROD parents closed to a fixed point in any order, unused BASE
    layers dropped (a remap that is not the identity); and a pair in which every layer is used (the
    identity remap, parents left as they are)."""
    rng = np.random.default_rng(0xDE04)
    a = _closure_cipher(rng)
    b = _mk(rng, 2, 4, at=(0, 1))
    every = np.arange(6000)
    c = _mk(rng, 6000, 200, at=every)   # BASE layers, each with an edge
    d = _mk(rng, 2, 2, at=(0, 1))
    eng = _engine(canon_tag=0xE1)
    out, plan, per, _, _ = _run_mul(eng, [a, c], [b, d], 4)
    assert eng.deep_path_counts()[0] == 2
    _check_pairs(oracle, out, [a, c], [b, d], per, canon_tag=0xE1)
    assert out[0].nL < a.nL + b.nL                      # unused layers went
    kept_prod = out[0].layers[out[0].layers["rule"] == 1]
    assert (kept_prod["pa"] < out[0].nL).all() and (kept_prod["pb"] < out[0].nL).all()
    assert out[1].nL == 6000 + 2 + 12000                # every layer kept: the identity


# ------------------------------------------------------------------ 5. cancellation
def test_cancelling_products(oracle):
    """Duplicate A edges (layer, idx, ch) with weights w and p - w: their products with any B edge sum
    to 0 mod p. Such cells are not emitted; a product layer with nothing else is dropped."""
    rng = np.random.default_rng(0xDE05)
    P = (1 << 127) - 1
    nl = 9000
    lay, idx, ch, lo, hi = [], [], [], [], []

    def edge(l, i, c, w):
        lay.append(l); idx.append(i); ch.append(c); lo.append(w & (2**64 - 1)); hi.append(w >> 64)

    gone, part = list(range(100, 150)), list(range(4000, 4050))
    for l in gone + part:
        w = int(rng.integers(1, 2**62)) | (int(rng.integers(0, 2**60)) << 64)
        i, c = int(rng.integers(0, B7)), int(rng.integers(0, 2))
        edge(l, i, c, w)
        edge(l, i, c, P - w)
        if l in part:   # and one edge that survives, in another cell
            edge(l, (i + 1) % B7, c, int(rng.integers(1, 2**62)))
    for l in rng.integers(5000, nl, 40).tolist():
        edge(l, int(rng.integers(0, B7)), int(rng.integers(0, 2)), int(rng.integers(1, 2**62)))
    order = rng.permutation(len(lay))
    a = Cipher(_base_layers(rng, nl), _meta(np.array(lay)[order], np.array(idx)[order], np.array(ch)[order]),
               np.array(lo, np.uint64)[order], np.array(hi, np.uint64)[order])
    b = _mk(rng, 1, 3)
    eng = _engine(canon_tag=0xE2)
    out, plan, per, _, _ = _run_mul(eng, [a], [b], 5)
    assert eng.deep_path_counts()[0] == 1
    ref = oracle.ct_mul(a, b, per[0], canon_tag=0xE2, Bm=B7)
    _same(out[0], ref)
    # the 50 fully cancelling A layers left no product layer (nor their BASE layer) behind
    kept = set(out[0].layers["nonce_lo"].tolist())
    assert not any(int(a.layers["nonce_lo"][l]) in kept for l in gone)
    assert all(int(a.layers["nonce_lo"][l]) in kept for l in part)


# ------------------------------------------------------------------ 6. order
def test_guard_budget_and_canonical_flag(oracle):
    """A deep pair above edge_budget = 500 comes out in the canonical (layer, idx, P<M) order with status
    1, and so does the same pair under PVAC_MUL_ORDER_CANONICAL with the default budget."""
    from pvac_hfhe_cppbyv_amd import MUL_ORDER_CANONICAL
    rng = np.random.default_rng(0xDE06)
    x, y = _mk(rng, 8192, 700), _mk(rng, 1, 3)
    eng = _engine(canon_tag=0xE3, edge_budget=500)
    out, plan, per, _, _ = _run_mul(eng, [x], [y], 6)
    assert out[0].nE > 500 and list(eng.ct_mul_status(1)) == [1]
    _same(out[0], oracle.ct_mul(x, y, per[0], canon_tag=0xE3, edge_budget=500, Bm=B7))
    eng2 = _engine(canon_tag=0xE3)
    out2, _, per2, _, _ = _run_mul(eng2, [x], [y], 6, flags=MUL_ORDER_CANONICAL)
    assert list(eng2.ct_mul_status(1)) == [1] and eng2.deep_path_counts()[0] == 1
    _same(out2[0], oracle.ct_mul(x, y, per2[0], canon_tag=0xE3, edge_budget=0, Bm=B7))
    _same(out2[0], out[0])


# ------------------------------------------------------------------ 7. rejection
def test_bad_layer_id_rejects_one_pair(oracle):
    """One edge with layer_id = |A.L| in the middle pair: status 2 and an empty output there, its
    neighbours bit-exact."""
    rng = np.random.default_rng(0xDE07)
    xs = [_mk(rng, 8192, 60) for _ in range(3)]
    ys = [_mk(rng, 1, 4) for _ in range(3)]
    bad = xs[1]
    bad.meta[17] = (bad.meta[17] & ~np.uint64(0xFFFFFFFF)) | np.uint64(bad.nL)
    eng = _engine(canon_tag=0xE4)
    out, plan, per, _, _ = _run_mul(eng, xs, ys, 7)
    assert list(eng.ct_mul_status(3)) == [0, 2, 0]
    assert out[1].nL == 0 and out[1].nE == 0
    _check_pairs(oracle, out, xs, ys, per, canon_tag=0xE4, skip=(1,))


# ------------------------------------------------------------------ 8. mixed batch
def test_mixed_batch_paths(oracle):
    """Fresh-shaped, ordinary general and deep pairs interleaved, through ct_mul_plan / ct_mul and through
    the one-call pvac_hip_ct_mul: bit-exact both ways, and the path counts say which pair went where."""
    rng = np.random.default_rng(0xDE08)
    kinds = ["fresh", "deep", "general", "fresh", "deep", "general", "deep"]
    # (fresh at B = 7: 28 key slots hold the bucket chains and sums of 4 x 4 products)
    mk = {"fresh": lambda: (_mk(rng, 2, 2, at=(0, 1)), _mk(rng, 2, 2, at=(0, 1))),
          "general": lambda: (_mk(rng, 100, 150), _mk(rng, 3, 12)),
          "deep": lambda: (_mk(rng, 8192 + int(rng.integers(0, 50)), 80), _mk(rng, 1 + int(rng.integers(0, 2)), 6))}
    pairs = [mk[k]() for k in kinds]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    eng = _engine(canon_tag=0xE5)
    out, plan, per, dev, _ = _run_mul(eng, xs, ys, 8)
    assert plan.n_small == 2 and plan.n_large == 5
    pc = eng.ct_mul_path_counts()
    assert (pc["fresh"], pc["general"]) == (2, 5) and eng.deep_path_counts()[0] == 3
    assert not eng.ct_mul_status(len(kinds)).any()
    _check_pairs(oracle, out, xs, ys, per, canon_tag=0xE5)
    # the one-call form into the same output arrays, the same nonces
    A, Bb, Cb, dn = dev
    for t in (Cb.layers, Cb.meta, Cb.w_lo, Cb.w_hi, Cb.l_cnt, Cb.e_cnt):
        t.zero_()
    plan2 = eng.ct_mul_into(A, Bb, Cb, dn)
    assert plan2.n_small == 2 and plan2.n_large == 5
    pc = eng.ct_mul_path_counts()
    assert (pc["fresh"], pc["general"]) == (4, 10) and eng.deep_path_counts()[0] == 6
    _check_pairs(oracle, Cb.to_host(), xs, ys, per, canon_tag=0xE5)


# ------------------------------------------------------------------ 9. sigma
def test_deep_pair_with_sigma(oracle, manifest, H_dense):
    """PVAC_MUL_WITH_SIGMA on one deep pair of fewer than 200 output edges: every sigma row equals the
    oracle's with the fixture H."""
    from pvac_hfhe_cppbyv_amd import MUL_WITH_SIGMA
    rng = np.random.default_rng(0xDE09)
    x, y = _mk(rng, 8192, 40), _mk(rng, 1, 2)
    eng = _engine(canon_tag=manifest["canon_tag"])
    assert eng.gen_H().hex() == manifest["H_digest"]
    out, plan, per, _, (salts, eoff) = _run_mul(eng, [x], [y], 9, flags=MUL_WITH_SIGMA, with_salts=True)
    assert 0 < out[0].nE < 200 and eng.deep_path_counts()[0] == 1
    ref = oracle.ct_mul(x, y, per[0], salts=salts[int(eoff[0]):], H=H_dense, canon_tag=manifest["canon_tag"], Bm=B7)
    _same(out[0], ref, sigma=True)


# ------------------------------------------------------------------ 10. limits
def test_layer_limit_api(oracle):
    """The default refuses (1, 8192) with "layers"; the setter takes DEFAULT .. MAX only; at 16,385 the
    engine accepts (1, 8192) and refuses (128, 128); the context stays usable."""
    from pvac_hfhe_cppbyv_amd import Engine, PvacError
    rng = np.random.default_rng(0xDE0A)
    x, y = _mk(rng, 1, 6), _mk(rng, 8192, 40)
    sq = _mk(rng, 128, 30)
    eng = Engine(device=0, B=B7, canon_tag=0xE6)
    assert eng.layer_limit == 16384
    with pytest.raises(PvacError, match="layers"):
        eng.ct_mul_plan(_dev_batch(eng, [x]), _dev_batch(eng, [y]))
    for bad in (16383, 2**24 + 1):
        assert eng.lib.pvac_hip_ctx_set_layer_limit(eng.ctx, bad) == -22
        with pytest.raises(PvacError, match="-22"):
            eng.set_layer_limit(bad)
        assert eng.layer_limit == 16384
    eng.set_layer_limit(2**24)
    assert eng.layer_limit == 2**24
    eng.set_layer_limit(16385)
    assert eng.layer_limit == 16385
    with pytest.raises(PvacError, match="16385 layers"):
        eng.ct_mul_plan(_dev_batch(eng, [sq]), _dev_batch(eng, [sq]))
    out, plan, per, _, _ = _run_mul(eng, [x], [y], 10)       # usable afterwards, and (1, 8192) runs
    _check_pairs(oracle, out, [x], [y], per, canon_tag=0xE6)
    assert eng.deep_path_counts() == (1, 0)
    eng.set_layer_limit(16384)                                # ... and back at the default it is refused again
    with pytest.raises(PvacError, match="16384 layers"):
        eng.ct_mul_plan(_dev_batch(eng, [x]), _dev_batch(eng, [y]))


# ------------------------------------------------------------------ 11. chain, 12. downstream
CHAIN_SEED, CHAIN_TAG = 0xC4A1, 0xE7


def _chain_inputs():
    rng = np.random.default_rng(0xDE0B)
    return [_mk(rng, 2, 0, at=(0, 1)) for _ in range(3)]   # 2 layers with 1 edge each


_LOOP = {}


def _oracle_loop(oracle, depth=14):
    """Input 0's chain c_k = ct_mul(c_{k-1}, x) on the CPU with the nonces pvac_hip_ct_mul_chain draws for
    chunk 0 (fill_random(seed + 97 * first_input + step) over the chunk's layer slots; input 0's slots
    come first): every c_k and the layers each step planned. Computed once."""
    if "c" not in _LOOP:
        x = _chain_inputs()[0]
        cs, planned = [x], []
        for d in range(depth):
            c = cs[-1]
            base, nn = c.nL + x.nL, 2 * c.nL * x.nL
            planned.append(base + c.nL * x.nL)
            words = splitmix_stream(CHAIN_SEED + d, 0, 2 * base + nn)
            cs.append(oracle.ct_mul(c, x, words[2 * base:], canon_tag=CHAIN_TAG, Bm=B7))
        _LOOP["c"], _LOOP["planned"] = cs, planned
    return _LOOP["c"], _LOOP["planned"]


def test_chain_depth_14(oracle):
    """The reference's loop c = ct_mul(pk, c, x) to depth 14 through ct_mul_chain (streams = 2, chunk = 2):
    steps 12 to 14 plan 24,638, 49,220 and about 98,000 layers. Final digests and counts of all three
    inputs equal the CPU port's chains, input 0's final cipher equals the oracle's loop in full, the gsum
    invariant holds on every pair-step, and a default engine fails the same call at step 12."""
    from pvac_hfhe_cppbyv_amd import ON_CHUNK_CB, Engine, PvacError, powg_table
    from helpers import hip_batch_to_host
    xs = _chain_inputs()
    cs, planned = _oracle_loop(oracle)
    assert planned[11:13] == [24638, 49220] and 97000 < planned[13] < 99000
    assert [cs[k].nL for k in (8, 9, 10, 11)] == [1038, 2064, 4114, 8212] and cs[13].nL == 32792
    eng = _engine(canon_tag=CHAIN_TAG)
    X = _dev_batch(eng, xs)
    got = {}

    def keep(user, first, cb, stream):
        got[first] = hip_batch_to_host(cb.contents, stream)
        return 0

    r = eng.ct_mul_chain(X, 14, nonce_seed=CHAIN_SEED, streams=2, chunk=2, digest_n=3, on_chunk=ON_CHUNK_CB(keep))
    assert r["chunks"] == 2 and r["pair_steps"] == 3 * 14
    assert eng.deep_path_counts()[0] == 3 * 3        # steps 12, 13, 14 of three inputs, on the workers
    px = pack_device_batch(X, 3)
    P_ = lambda a: a.ctypes.data_as(C.c_void_p)
    ocnt, odig, se = np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(14, np.uint64)
    oracle.lib.orc_ct_mul_chain_timed(C.byref(default_params(CHAIN_TAG, B=B7)), 3, *(P_(a) for a in px), 14, 8,
                                      P_(ocnt), P_(odig), P_(se))
    assert np.array_equal(r["digests"], odig) and np.array_equal(r["counts"], ocnt)
    assert r["edges"] == [int(v) for v in se]
    _same(got[0][0], cs[14])
    eng.set_powg(powg_table(B7))
    r2 = eng.ct_mul_chain(X, 14, nonce_seed=CHAIN_SEED, streams=2, chunk=2, digest_n=3, check_gsum=True)
    assert r2["gsum_pairs"] == 3 * 14 and r2["gsum_failed"] == 0
    assert np.array_equal(r2["digests"], odig)
    dflt = Engine(device=0, B=B7, canon_tag=CHAIN_TAG)
    Xd = _dev_batch(dflt, xs)
    with pytest.raises(PvacError, match="more than 16384 layers"):
        dflt.ct_mul_chain(Xd, 14, nonce_seed=CHAIN_SEED, streams=2, chunk=2, digest_n=3)
    ok = dflt.ct_mul_chain(Xd, 11, nonce_seed=CHAIN_SEED, streams=2, chunk=2, digest_n=3)   # step 11 still runs
    assert ok["pair_steps"] == 33


def test_downstream_of_a_deep_product(oracle):
    """The depth-13 product (32,792 layers) goes on: ct_add and ct_sub with itself (65,584 layers, the deep
    ct_add kernel, counted), a sigma-carrying add above 30,000 layers, dec_value, commit_ct, and a
    ct_image / ct_from_image round trip."""
    from pvac_hfhe_cppbyv_amd import powg_table
    cs, _ = _oracle_loop(oracle)
    c13 = cs[13]
    assert c13.nL == 32792
    eng = _engine(canon_tag=CHAIN_TAG)
    X = _dev_batch(eng, [c13])
    for k, neg in enumerate((False, True)):
        S = eng.ct_add(X, X, negate=neg)
        assert eng.deep_path_counts() == (0, k + 1)
        ref = oracle.ct_add(c13, c13, negate=neg)
        assert ref.nL == 2 * 32792
        _same(S.to_host()[0], ref)
    # a call under 30,001 layers stays on k_ct_add
    small = _dev_batch(eng, [cs[11]])
    _same(eng.ct_add(small, small).to_host()[0], oracle.ct_add(cs[11], cs[11]))
    assert eng.deep_path_counts() == (0, 2)
    # sigma rows through the deep kernel: 15,001 + 15,001 layers, some unused
    rng = np.random.default_rng(0xDE0C)
    u, v = _mk(rng, 15001, 30, at=(0, 15000)), _mk(rng, 15001, 30, at=(0, 15000))
    for c in (u, v):
        c.sigma = rng.integers(0, 2**63, (c.nE, 128), dtype=np.uint64)
    got = eng.ct_add(_dev_batch(eng, [u], sigma=True), _dev_batch(eng, [v], sigma=True), sigma=True).to_host()[0]
    _same(got, oracle.ct_add(u, v), sigma=True)
    assert eng.deep_path_counts() == (0, 3) and got.nL < 30002
    # dec_value with random R on the BASE layers
    powg = powg_table(B7)
    eng.set_powg(powg)
    R = rng.integers(1, 2**62, 2 * c13.nL, dtype=np.uint64)
    vals, st = eng.dec_value(X, R)
    assert not st.any()
    lo, hi = oracle.dec(c13, powg, R)
    assert vals[0] == lo | (hi << 64)
    # commit_ct
    hd = bytes(range(32))
    eng.set_H_digest(hd)
    assert eng.commit_ct(X, with_sigma=False)[0].tobytes() == oracle.commit(c13, CHAIN_TAG, hd)
    # the device codec
    image, pos = eng.ct_image(X, 8192, return_pos=True)
    Y = eng.ct_from_image(image, pos, 1, 0, c13.nL, c13.nE, sigma=False)
    back = Y.to_host()[0]
    for f in ("rule", "pa", "pb"):
        assert np.array_equal(back.layers[f], c13.layers[f])
    base = c13.layers["rule"] == 0   # a .ct file keeps the seeds of BASE layers only
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(back.layers[f][base], c13.layers[f][base])
    assert np.array_equal(back.meta, c13.meta) and np.array_equal(back.w_lo, c13.w_lo) and np.array_equal(back.w_hi, c13.w_hi)
