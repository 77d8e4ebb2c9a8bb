"""GPU parity of ct_lincomb / ct_sum, compact and ct_recrypt on ciphers of more than 30,000 layers, accepted
under a raised per-context layer limit (Engine(layer_limit=...)): the deep-term route of ct_lincomb
(k_lincomb_plan_deep: keep and remap words in global scratch), its fold route on k_ct_add_deep and the merge
kernel, compact's merge path and ct_recrypt's sums. Every output cipher is compared in full with the CPU
models (tests/lincomb_model.py, tests/recrypt_model.py, both on the pinned oracle's ct_add): layer records
with remapped parents, metas, both weight words, and sigma rows where carried. The ciphers are many layer
records and a few dozen edges (30,001 layers are 1.2 MB); B = 7 keeps compact's key space small."""
import re

import numpy as np
import pytest

import lincomb_model as lm
import recrypt_model as rm
from helpers import LAYER_DT, Cipher

pytestmark = pytest.mark.gpu

B7 = 7
LIMIT = 1 << 17
P = (1 << 127) - 1
M64 = (1 << 64) - 1
TAG = 0xD0


def _engine(**kw):
    from pvac_hfhe_cppbyv_amd import Engine
    kw.setdefault("B", B7)
    kw.setdefault("layer_limit", LIMIT)
    kw.setdefault("canon_tag", TAG)
    return Engine(device=0, **kw)


def _dev_batch(eng, ciphers, sigma=False):
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    hc = [HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in ciphers]
    return DeviceBatch.from_host(hc, eng.device, sigma=sigma)


def _same(got, ref, sigma=False):
    for f in ("rule", "pa", "pb", "ztag", "nonce_lo", "nonce_hi"):
        assert np.array_equal(got.layers[f], ref.layers[f]), f
    assert got.nE == ref.nE
    assert np.array_equal(got.meta, ref.meta)
    assert np.array_equal(got.w_lo, ref.w_lo) and np.array_equal(got.w_hi, ref.w_hi)
    if sigma:
        assert got.sigma is not None and np.array_equal(np.asarray(got.sigma).reshape(got.nE, -1),
                                                        np.asarray(ref.sigma).reshape(ref.nE, -1))


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


def _prod(L, l, pa, pb):
    L[l]["rule"], L[l]["pa"], L[l]["pb"] = 1, pa, pb
    L[l]["ztag"] = L[l]["nonce_lo"] = L[l]["nonce_hi"] = 0


def _tree(rng, nl, ne=12):
    """nl layers as a heap: layer l is the PROD of 2l + 1 and 2l + 2 while those exist. An edge on layer 0
    keeps every layer (the identity remap) through a closure about log2(nl) levels deep."""
    L = _base_layers(rng, nl)
    for l in range(nl):
        if 2 * l + 1 < nl:
            _prod(L, l, 2 * l + 1, min(2 * l + 2, nl - 1))
    return _mk(rng, nl, ne, at=(0,), layers=L)


def _chained(rng, nl=30010):
    """Edges only on PROD layer 30005; its parents lead back through PROD layers 30003, 29990 and 15000 to
    BASE layers 1, 2, 3 and 29999, 30008: each link points to a lower index, and one to a higher one, so no
    single sweep closes it. Nine layers stay."""
    L = _base_layers(rng, nl)
    _prod(L, 30005, 30003, 3)
    _prod(L, 30003, 29990, 30008)
    _prod(L, 29990, 15000, 29999)
    _prod(L, 15000, 1, 2)
    return _mk(rng, nl, 0, at=[30005] * 20, layers=L)


def _with_sigma(rng, c, zero=False):
    s = np.zeros((c.nE, 128), np.uint64) if zero else rng.integers(0, 2**64 - 1, (c.nE, 128), dtype=np.uint64, endpoint=True)
    return Cipher(c.layers, c.meta, c.w_lo, c.w_hi, s)


def _lincomb(eng, oracle, pool, segs, scales=None, flags=None, sigma=False, edge_budget=1200000):
    """One ct_lincomb call over `segs` (lists of pool indices); every output against the model's fold."""
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    term = np.array([t for s in segs for t in s], np.uint64)
    out = eng.ct_lincomb(_dev_batch(eng, pool, sigma=sigma), seg_off, term, scales, flags, sigma=sigma).to_host()
    want = lm.fold_segments(oracle, pool, seg_off, term, scales, flags, edge_budget=edge_budget, sigma=sigma)
    assert len(out) == len(want)
    for g, w in zip(out, want):
        _same(g, w, sigma=sigma)
    return out


# ------------------------------------------------------------------ 1. boundary
def test_boundary_30000_and_30001(oracle):
    """One ct_sum call: the 30,000-layer term is the workgroup route's (LDS keep table), the 30,001-layer term
    the deep-term route's. Both equal the model."""
    rng = np.random.default_rng(0xD001)
    pool = [_mk(rng, 30000, 40, at=(0, 29999)), _mk(rng, 30001, 40, at=(0, 30000))]
    eng = _engine()
    assert eng.deep_route_counts() == (0, 0, 0, 0)
    seg_off = np.array([0, 1, 2], np.uint64)
    out = eng.ct_sum(_dev_batch(eng, pool), seg_off).to_host()
    for k, g in enumerate(out):
        _same(g, lm.fold(oracle, pool, [k]))
    pc = eng.ct_lincomb_path_counts()
    assert (pc["one_pass"], pc["fold"], pc["wave_terms"], pc["wg_terms"]) == (2, 0, 0, 1)
    assert eng.deep_route_counts() == (1, 0, 0, 0)
    assert not eng.ct_lincomb_status(2).any()


# ------------------------------------------------------------------ 2. closure and remap
def test_deep_term_closure_and_remap(oracle):
    """Three deep terms, each alone in a segment (ct_add({}, t)) and as the middle term of a segment between
    two shallow ones (its layer offset and its edges' offset are not 0): a closure of several passes that keeps
    nine layers, a term that keeps every layer (the identity remap) and one that keeps its edges' layers only."""
    rng = np.random.default_rng(0xD002)
    chained, every, own = _chained(rng), _tree(rng, 30001), _mk(rng, 30040, 30)
    left, right = _mk(rng, 3, 8, at=(0, 2)), _mk(rng, 70, 25)
    pool = [chained, every, own, left, right]
    segs = [[0], [1], [2], [3, 0, 4], [3, 1, 4], [3, 2, 4]]
    eng = _engine()
    out = _lincomb(eng, oracle, pool, segs)
    assert out[0].nL == 9 and out[1].nL == 30001 and out[2].nL == len(np.unique(own.layer_id()))
    assert out[4].nL == 30001 + out[3].nL - 9
    pc = eng.ct_lincomb_path_counts()
    assert (pc["one_pass"], pc["fold"], pc["wave_terms"], pc["wg_terms"]) == (6, 0, 3, 3)   # `right` has 70 layers
    assert eng.deep_route_counts() == (6, 0, 0, 0)


# ------------------------------------------------------------------ 3. a deep term twice, scales, sigma
def test_deep_term_twice_scaled_and_sigma(oracle):
    """One deep cipher is a term twice in a segment: scaled by p - 1 (ct_neg) and unscaled, its raw weight
    words (a non-canonical one among them) carried as they are. The same call again with sigma rows."""
    rng = np.random.default_rng(0xD003)
    deep = _mk(rng, 30050, 24, full=True)
    deep.w_lo[0], deep.w_hi[0] = np.uint64(M64), np.uint64(M64)   # a word above p
    pool = [_with_sigma(rng, deep), _with_sigma(rng, _mk(rng, 5, 9))]
    segs = [[0, 1, 0]]
    scales, flags = [P - 1, 1, 1], np.array([1, 0, 0], np.uint32)
    eng = _engine()
    out = _lincomb(eng, oracle, pool, segs, scales, flags)
    assert int(out[0].w_lo[-24]) == M64 and int(out[0].w_hi[-24]) == M64   # the second use: raw
    _lincomb(eng, oracle, pool, segs, scales, flags, sigma=True)
    assert eng.deep_route_counts() == (4, 0, 0, 0)


# ------------------------------------------------------------------ 4. the fold route
def _fold_pool(rng):
    """A 2-layer term with an edge on layer 3 (out of contract: in the fold it lands on the next term's layer
    1) and two heaps of 16,000 layers, which ct_add keeps whole: the running sum passes 30,000 layers."""
    stray = _mk(rng, 2, 0, at=(0, 1, 0, 3, 1))
    return [stray, _tree(rng, 16000), _tree(rng, 16000)]


def test_fold_route_deep_sum(oracle):
    rng = np.random.default_rng(0xD004)
    pool = _fold_pool(rng)
    eng = _engine()
    out = _lincomb(eng, oracle, pool, [[0, 1, 2]])
    assert out[0].nL == 32002
    assert list(eng.ct_lincomb_status(1)) == [2]
    assert eng.deep_route_counts()[1] == 1 and eng.deep_path_counts()[1] == 1   # the last sum: 16,002 + 16,000
    assert eng.ct_lincomb_path_counts()["fold"] == 1


def test_fold_route_deep_sum_over_budget(oracle):
    """edge_budget = 10: the same segment is over budget, and every sum goes through the merge kernel
    (guard_budget: the canonical edge order)."""
    rng = np.random.default_rng(0xD004)
    pool = _fold_pool(rng)
    eng = _engine(edge_budget=10)
    out = _lincomb(eng, oracle, pool, [[0, 1, 2]], edge_budget=10)
    assert list(eng.ct_lincomb_status(1)) == [1]
    m = out[0].meta
    key = (m & np.uint64(0xFFFFFFFF)) << np.uint64(20) | ((m >> np.uint64(32)) & np.uint64(0xFFFF)) << np.uint64(1) | (m >> np.uint64(48))
    assert (np.diff(key.astype(np.int64)) > 0).all()


# ------------------------------------------------------------------ 5. compact
def _compact_cipher(rng, nl):
    """nl layers (the last one a PROD of layers 5 and nl - 2), sigma rows, duplicate (layer, idx, ch) edges; on
    layer 123 a pair whose weights cancel and whose sigmas are equal (dropped, and the layer with it), on layer
    456 a pair whose weights cancel and whose sigmas differ (kept with weight 0)."""
    L = _base_layers(rng, nl)
    _prod(L, nl - 1, 5, nl - 2)
    c = _mk(rng, nl, 40, at=(nl - 1, 0), layers=L)
    keep = ~np.isin(c.layer_id(), (123, 456))
    meta, lo, hi = list(c.meta[keep]), list(c.w_lo[keep]), list(c.w_hi[keep])
    for k in range(10):   # duplicates of the first ten edges, other weights
        meta.append(meta[k]); lo.append(int(rng.integers(0, 2**63))); hi.append(int(rng.integers(0, 2**62)))
    sg = [rng.integers(0, 2**63, 128, dtype=np.uint64) for _ in meta]
    for lid, same_sigma in ((123, True), (456, False)):
        w = int(rng.integers(1, 2**62)) | (int(rng.integers(1, 2**60)) << 64)
        s = rng.integers(0, 2**63, 128, dtype=np.uint64)
        for v, sv in ((w, s), (P - w, s if same_sigma else rng.integers(0, 2**63, 128, dtype=np.uint64))):
            meta.append(int(_meta(lid, 2, 1))); lo.append(v & M64); hi.append(v >> 64); sg.append(sv)
    order = rng.permutation(len(meta))
    take = lambda a: np.array(a, np.uint64)[order]
    return Cipher(L, take(meta), take(lo), take(hi), np.array(sg, np.uint64)[order])


def test_compact_deep(oracle):
    rng = np.random.default_rng(0xD005)
    cs = [_compact_cipher(rng, 30001), _compact_cipher(rng, 30000)]
    eng = _engine()
    out = eng.compact(_dev_batch(eng, cs, sigma=True)).to_host()
    for g, c in zip(out, cs):
        ref = rm.compact(oracle, c)
        _same(g, ref, sigma=True)
        kept = set(g.layers["nonce_lo"].tolist())
        assert int(c.layers["nonce_lo"][123]) not in kept and int(c.layers["nonce_lo"][456]) in kept
        assert g.nE < c.nE - 2 and g.nL < 60
        assert g.layers["rule"][-1] == 1 and g.layers["pa"][-1] < g.nL and g.layers["pb"][-1] == g.nL - 2
    assert eng.compact_path_counts() == {"small": 0, "merge": 2}   # the 30,000-layer neighbour: the merge path, as before
    assert eng.deep_route_counts() == (0, 0, 1, 0)


# ------------------------------------------------------------------ 6. ct_recrypt
def test_recrypt_deep(oracle):
    """Inputs and pool with all-zero sigma rows: the density stays 0, so all eight iterations run. The heaps
    keep every layer through each ct_add. From 30,001 layers all eight sums are above 30,000; from 29,990, with
    two layers per pool member, the sums are 29,992 + 2 it: the last three."""
    rng = np.random.default_rng(0xD006)
    pool = [_with_sigma(rng, _mk(rng, 2, 4, at=(0, 1)), zero=True) for _ in range(3)]
    picks = np.array([2, 0, 1, 1, 2**63 + 5, 0, 2, 1], np.uint64)
    inv = rm.gen_ubk(TAG, 8192)[1]
    eng = _engine()
    eng.set_ubk(inv)
    Pb = _dev_batch(eng, pool, sigma=True)
    for nl, sums, compacted in ((30001, 8, 1), (29990, 11, 2)):
        x = _with_sigma(rng, _tree(rng, nl, ne=20), zero=True)
        want, its = rm.recrypt(oracle, x, pool, picks, inv)
        assert its == 8 and want.nL == nl + 16
        out, iters = eng.ct_recrypt(_dev_batch(eng, [x], sigma=True), Pb, picks)
        assert list(iters) == [8]
        _same(out.to_host()[0], want, sigma=True)
        assert eng.deep_route_counts() == (0, 0, compacted, sums)


# ------------------------------------------------------------------ 7. the default limit
def test_default_limit_refuses_as_before(oracle):
    """At the default layer limit each call is refused with PVAC_ENOSYS and the message it always had, and
    nothing is counted."""
    from pvac_hfhe_cppbyv_amd import Engine, PvacError
    rng = np.random.default_rng(0xD007)
    eng = Engine(device=0, B=B7, canon_tag=TAG)
    assert eng.layer_limit == 16384

    def refused(msg, call):
        with pytest.raises(PvacError, match=re.escape("error -38: " + msg) + "$"):
            call()

    pool = [_mk(rng, 30000, 40), _mk(rng, 30001, 40)]
    X = _dev_batch(eng, pool)
    refused("ct_lincomb_plan: a term above 30000 layers", lambda: eng.ct_sum(X, np.array([0, 1, 2], np.uint64)))
    cs = [_with_sigma(rng, _mk(rng, 30001, 30)), _with_sigma(rng, _mk(rng, 30000, 30))]
    refused("compact_plan: a cipher beyond 30000 layers, 2^31 edges or 2^32 keys",
            lambda: eng.compact(_dev_batch(eng, cs, sigma=True)))
    eng.set_ubk(rm.gen_ubk(TAG, 8192)[1])
    zp = [_with_sigma(rng, _mk(rng, 2, 4, at=(0, 1)), zero=True)]
    x = _with_sigma(rng, _tree(rng, 30001), zero=True)
    refused("ct_add_exec: > 30000 layers per cipher",
            lambda: eng.ct_recrypt(_dev_batch(eng, [x], sigma=True), _dev_batch(eng, zp, sigma=True), np.zeros(8, np.uint64)))
    assert eng.deep_route_counts() == (0, 0, 0, 0)
    # the context stays usable, and the 30,000-layer neighbours pass as they did
    _same(eng.ct_sum(_dev_batch(eng, pool[:1]), np.array([0, 1], np.uint64)).to_host()[0], lm.fold(oracle, pool, [0]))
    _same(eng.compact(_dev_batch(eng, cs[1:], sigma=True)).to_host()[0], rm.compact(oracle, cs[1]), sigma=True)
    assert eng.deep_route_counts() == (0, 0, 0, 0)


# ------------------------------------------------------------------ 8. the real shape
def test_sum_of_chain_products(oracle):
    """The reference's loop c = ct_mul(pk, c, x): its depth-13 cipher (32,792 layers) summed with itself and
    the depth-11 cipher (8,212 layers) in one ct_sum. No sigma is carried."""
    from test_gpu_deep import _oracle_loop
    cs, _ = _oracle_loop(oracle)
    pool = [cs[13], cs[11]]
    assert pool[0].nL == 32792 and pool[1].nL == 8212
    eng = _engine(canon_tag=0xE7)
    out = _lincomb(eng, oracle, pool, [[0, 0, 1]])
    assert out[0].nL == 2 * 32792 + 8212
    assert eng.deep_route_counts()[0] == 2 and eng.ct_lincomb_path_counts()["wg_terms"] == 1
