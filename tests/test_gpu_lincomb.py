"""GPU parity of the batched ct_lincomb (k_lincomb.hip, rt_lincomb.cpp): segmented sums of optionally
scaled ciphers against the reference-minted digests of tests/golden/lincomb and against the model of
tests/lincomb_model.py (the reference's fold on the CPU oracle's ct_add), byte for byte, over the
shapes at which the term routes, the segment bookkeeping, the scaling, the sigma carry, the split of a
large term over workgroups and the fold route can go wrong."""
import numpy as np
import pytest

import lincomb_model as lm
from helpers import LAYER_DT, Cipher, pack_meta

pytestmark = pytest.mark.gpu

EINVAL, ENOSYS = "error -22", "error -38"


def make_engine(**kw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, **kw)


@pytest.fixture(scope="module")
def eng():
    return make_engine()


@pytest.fixture(scope="module")
def eng100():
    """edge_budget = 100: three fresh ciphers are over budget."""
    return make_engine(edge_budget=100)


def dev(engine, ciphers, sigma=False):
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    return DeviceBatch.from_host(ciphers, engine.device, sigma=sigma)


def host(batch):
    return [Cipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in batch.to_host()]


def check(got, want, sigma=False):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.nL, g.nE) == (w.nL, w.nE), i
        assert lm.same(g, w, sigma), i


def synthetic(rng, n_layers, n_edges):
    """A cipher inside the contract with every kind of layer compact_layers tells apart: every fifth
    layer from 2 on is a PROD of two earlier layers, about 60% of the layers carry edges, and (from 6
    layers on) the last layer is an unused PROD whose parents nothing else uses."""
    layers = np.zeros(n_layers, LAYER_DT)
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        layers[f] = rng.integers(0, 2**63, n_layers, dtype=np.uint64)
    top = n_layers - 3 if n_layers >= 6 else n_layers
    for l in range(2, top, 5):
        layers[l] = (1, rng.integers(0, l), rng.integers(0, l), 0, 0, 0, 0)
    if n_layers >= 6:
        layers[n_layers - 1] = (1, n_layers - 2, n_layers - 3, 0, 0, 0, 0)
    with_edges = np.flatnonzero(rng.random(top) < 0.6).astype(np.uint64)
    if not len(with_edges):
        with_edges = np.array([0], np.uint64)
    lid = with_edges[rng.integers(0, len(with_edges), n_edges)]
    meta = pack_meta(lid, rng.integers(0, 337, n_edges), rng.integers(0, 2, n_edges))
    return Cipher(layers, meta, rng.integers(0, 2**64, n_edges, dtype=np.uint64),
                  rng.integers(0, 2**63, n_edges, dtype=np.uint64))


# ---------------------------------------------------------------- the reference's digests
_GOLDEN_ENGINES = {}


@pytest.mark.parametrize("name", [c["name"] for c in lm.manifest()["cases"]])
def test_golden(name):
    man = lm.manifest()
    case = next(c for c in man["cases"] if c["name"] == name)
    budget = case["edge_budget"]
    if budget not in _GOLDEN_ENGINES:
        e = make_engine(canon_tag=man["canon_tag"], edge_budget=budget)
        e.set_H_digest(bytes.fromhex(man["H_digest"]))
        _GOLDEN_ENGINES[budget] = e
    e = _GOLDEN_ENGINES[budget]
    pool, term, scales, flags = lm.case_inputs(case)
    before = e.ct_lincomb_path_counts()
    sigma = case["sigma"] and len(pool) > 0   # no rows to carry from an empty pool
    X = dev(e, pool, sigma=sigma)
    out = e.ct_lincomb(X, [0, len(term)], term, scales, flags, sigma=sigma)
    got = host(out)[0]
    assert (got.nL, got.nE) == (case["out_layers"], case["out_edges"])
    assert e.commit_ct(out, with_sigma=sigma)[0].tobytes().hex() == case["commit"]
    after = e.ct_lincomb_path_counts()
    fold = 1 if name == "guard" else 0
    assert after["fold"] - before["fold"] == fold and after["one_pass"] - before["one_pass"] == 1 - fold
    assert list(e.ct_lincomb_status(1)) == [fold]


# ---------------------------------------------------------------- segment bookkeeping
def test_segments(eng, oracle):
    rng = np.random.default_rng(0x5E6)
    g = lm.golden_cipher
    pool = [lm.strip(c) for c in host(eng.gen_fresh(40, 0x11))]
    pool += [lm.strip(g(f"ref/enc{i}.ct")) for i in range(8)]
    pool += [lm.empty_cipher() for _ in range(4)]
    pool += [lm.strip(g("lincomb/unused_in.ct"))] * 4
    pool += [synthetic(rng, 7, 30) for _ in range(8)]
    assert len(pool) == 64
    # a leading and a trailing empty segment, two adjacent empty ones
    lens = [0, 1, 2, 3, 0, 0, 31, 32, 33, 63, 64, 65, 257, 0]
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    term = rng.integers(0, 64, int(seg_off[-1])).astype(np.uint64)
    a, b = int(seg_off[7]), int(seg_off[12])
    term[a:a + 4] = 5              # one cipher four times in a row
    term[b + 100:b + 110] = 52     # the cipher with an unused layer, repeated
    X = dev(eng, pool)
    out = eng.ct_sum(X, seg_off, term)
    check(host(out), lm.fold_segments(oracle, pool, seg_off, term))
    assert not eng.ct_lincomb_status(len(lens)).any()
    # consecutive ciphers: term = None
    so2 = np.array([0, 3, 3, 64], np.uint64)
    check(host(eng.ct_sum(X, so2)), lm.fold_segments(oracle, pool, so2, np.arange(64)))


# ---------------------------------------------------------------- term routes
def test_layer_routes(eng, oracle):
    rng = np.random.default_rng(0x1A7)
    sizes = [1, 32, 33, 64, 65, 70, 1000]
    pool = [synthetic(rng, L, 3 * L + 5) for L in sizes] + [lm.strip(c) for c in host(eng.gen_fresh(3, 0x12))]
    # all in one segment (twice, in two orders), each alone, and mixed small groups
    segs = [list(range(10)), [6, 4, 2, 0, 9, 1, 3, 5]] + [[k] for k in range(7)] + [[4, 0, 6, 2], [7, 3], [1, 8, 1], [5, 5]]
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    term = np.array([t for s in segs for t in s], np.uint64)
    before = eng.ct_lincomb_path_counts()
    out = eng.ct_sum(dev(eng, pool), seg_off, term)
    check(host(out), lm.fold_segments(oracle, pool, seg_off, term))
    after = eng.ct_lincomb_path_counts()
    n_wg = int(sum(1 for t in term if pool[int(t)].nL > 64))
    assert after["wg_terms"] - before["wg_terms"] == n_wg > 0
    assert after["wave_terms"] - before["wave_terms"] == len(term) - n_wg > 0
    assert after["fold"] == before["fold"]


# ---------------------------------------------------------------- scales
def test_scales(eng, oracle):
    pool = [lm.strip(lm.golden_cipher(f"ref/fr{i}_x.ct")) for i in range(5)]
    consts = [0, 1, lm.P - 1, lm.P, 2**128 - 1]
    # every cipher with every scale and unscaled, scaled and unscaled terms side by side
    term, scales, flags = [], [], []
    for t in range(5):
        for s in consts:
            term += [t, t]
            scales += [s, s]
            flags += [1, 0]
    seg_off = np.arange(0, len(term) + 1, 10, dtype=np.uint64)
    X = dev(eng, pool)
    out = host(eng.ct_lincomb(X, seg_off, term, scales, np.array(flags, np.uint32)))
    check(out, lm.fold_segments(oracle, pool, seg_off, term, scales, flags))
    for t in range(5):   # the unscaled rows are the inputs' raw words
        c, e = out[t], 0
        for k in range(10):
            n = pool[t].nE
            if k % 2:
                assert np.array_equal(c.w_lo[e:e + n], pool[t].w_lo) and np.array_equal(c.w_hi[e:e + n], pool[t].w_hi)
            e += n
    # flags = None: every term is scaled
    out = host(eng.ct_lincomb(X, seg_off, term, scales))
    check(out, lm.fold_segments(oracle, pool, seg_off, term, scales))


# ---------------------------------------------------------------- sigma rows
def test_sigma(eng, oracle):
    pool = [lm.golden_cipher(f"ref/enc{i}.ct") for i in range(6)]
    seg_off = np.array([0, 3, 4, 9], np.uint64)
    term = np.array([0, 1, 2, 3, 4, 5, 4, 0, 2], np.uint64)
    X = dev(eng, pool, sigma=True)
    out = host(eng.ct_sum(X, seg_off, term, sigma=True))
    check(out, lm.fold_segments(oracle, pool, seg_off, term, sigma=True), sigma=True)
    for i in range(3):   # the rows are the inputs' rows at their new positions
        rows = np.concatenate([pool[int(t)].sigma for t in term[int(seg_off[i]):int(seg_off[i + 1])]])
        assert np.array_equal(out[i].sigma, rows)
    plain = host(eng.ct_sum(X, seg_off, term, sigma=False))
    assert all(c.sigma is None for c in plain)
    check(plain, [lm.strip(c) for c in out])


# ---------------------------------------------------------------- one large term over many workgroups
def test_big_term(eng):
    rng = np.random.default_rng(0xB16)
    n = 200_003
    layers = np.zeros(3, LAYER_DT)
    layers["ztag"] = [11, 12, 13]
    lid = rng.integers(0, 2, n).astype(np.uint64) * np.uint64(2)   # layer 1 is unused
    big = Cipher(layers, pack_meta(lid, rng.integers(0, 337, n), rng.integers(0, 2, n)),
                 rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**63, n, dtype=np.uint64))
    small = [lm.strip(c) for c in host(eng.gen_fresh(4, 0x13))]
    pool = small[:2] + [big] + small[2:]
    out = host(eng.ct_sum(dev(eng, pool), [0, 5], np.arange(5)))[0]
    # the concatenation, in numpy: two layers per small cipher, layers 0 and 2 of the large one
    want_layers = np.concatenate([small[0].layers, small[1].layers, layers[[0, 2]], small[2].layers, small[3].layers])
    big_meta = (big.meta & np.uint64(0xFFFFFFFF00000000)) | (lid // np.uint64(2) + np.uint64(4))
    metas = [small[0].meta, small[1].meta + np.uint64(2), big_meta, small[2].meta + np.uint64(6), small[3].meta + np.uint64(8)]
    assert out.layers.tobytes() == want_layers.tobytes()
    assert np.array_equal(out.meta, np.concatenate(metas))
    assert np.array_equal(out.w_lo, np.concatenate([c.w_lo for c in pool]))
    assert np.array_equal(out.w_hi, np.concatenate([c.w_hi for c in pool]))


# ---------------------------------------------------------------- the fold route
def test_fold_routes(eng100, oracle):
    rng = np.random.default_rng(0xF01D)
    fresh = [lm.strip(c) for c in host(eng100.gen_fresh(6, 0x14))]
    # out of contract: an edge of a 2-layer cipher points at layer 3, which is the second layer of the
    # term that follows it in the sum (a layer nothing else uses: only the fold keeps it)
    def two_layers(n_edges, lid):
        layers = np.zeros(2, LAYER_DT)
        layers["ztag"] = rng.integers(0, 2**63, 2, dtype=np.uint64)
        meta = pack_meta(lid, rng.integers(0, 337, n_edges), rng.integers(0, 2, n_edges))
        return Cipher(layers, meta, rng.integers(0, 2**64, n_edges, dtype=np.uint64),
                      rng.integers(0, 2**63, n_edges, dtype=np.uint64))

    stray = two_layers(12, [0, 1, 0, 1, 0, 3, 0, 1, 0, 1, 0, 1])
    partner = two_layers(9, [0] * 9)
    pool = fresh + [stray, partner]
    segs = [[0, 1], [0, 1, 2], [6, 7], [3], [2, 3, 4, 5], []]
    want_status = [0, 1, 2, 0, 1, 0]
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    term = np.array([t for s in segs for t in s], np.uint64)
    scales = [lm.P - 1 if k % 3 == 0 else 7 for k in range(len(term))]
    flags = np.array([k % 2 for k in range(len(term))], np.uint32)
    before = eng100.ct_lincomb_path_counts()
    out = host(eng100.ct_lincomb(dev(eng100, pool), seg_off, term, scales, flags))
    want = lm.fold_segments(oracle, pool, seg_off, term, scales, flags, edge_budget=100)
    assert want[2].nL == 4   # the stray edge kept the partner's unused layer
    check(out, want)
    assert list(eng100.ct_lincomb_status(len(segs))) == want_status
    after = eng100.ct_lincomb_path_counts()
    assert after["fold"] - before["fold"] == 3 and after["one_pass"] - before["one_pass"] == 3


# ---------------------------------------------------------------- against ct_add itself
def test_matches_ct_add(eng):
    n = 300
    A, B = eng.gen_fresh(n, 0x15), eng.gen_fresh(n, 0x16)
    X = dev(eng, host(A) + host(B))
    seg_off = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    term = np.stack([np.arange(n), np.arange(n) + n], axis=1).reshape(-1).astype(np.uint64)
    check(host(eng.ct_sum(X, seg_off, term)), host(eng.ct_add(A, B)))
    flags = np.tile(np.array([0, 1], np.uint32), n)
    got = host(eng.ct_lincomb(X, seg_off, term, [lm.P - 1] * (2 * n), flags))
    check(got, host(eng.ct_add(A, B, negate=True)))


# ---------------------------------------------------------------- rejections leave C alone
def test_errors(eng):
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch, PvacError
    pool = [lm.strip(c) for c in host(eng.gen_fresh(4, 0x17))]
    X = dev(eng, pool)

    def prefilled(n=2):
        f = lambda *shape: torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=eng.device)
        return DeviceBatch(n, f(n), f(n), f(64, 5), f(n), f(n), f(512), f(512), f(512))

    def snapshot(c):
        return [t.clone() for t in (c.l_off, c.l_cnt, c.layers, c.e_off, c.e_cnt, c.meta, c.w_lo, c.w_hi)]

    def untouched(c, snap):
        return all(torch.equal(a, b) for a, b in zip(snapshot(c), snap))

    for seg_off, term in (([0, 3, 2], [0, 1, 2]),      # decreasing
                          ([1, 2, 3], [0, 1, 2]),      # does not start at 0
                          ([0, 1, 2], [0, 1, 2]),      # does not end at n_terms
                          ([0, 2, 3], [0, 4, 1])):     # term index = X.n
        C_ = prefilled()
        snap = snapshot(C_)
        with pytest.raises(PvacError, match=EINVAL):
            eng.ct_lincomb_plan(X, seg_off, term, C_=C_)
        assert untouched(C_, snap)
    # a term of 30,001 layers
    layers = np.zeros(30001, LAYER_DT)
    giant = Cipher(layers, pack_meta([0, 30000], [1, 2], [0, 1]), np.array([1, 2], np.uint64), np.array([0, 0], np.uint64))
    C_ = prefilled()
    snap = snapshot(C_)
    with pytest.raises(PvacError, match=ENOSYS):
        eng.ct_lincomb_plan(dev(eng, pool + [giant]), [0, 1, 2], [0, 4], C_=C_)
    assert untouched(C_, snap)
    # a stale plan: any later plan of the context
    C1, plan1, call1 = eng.ct_lincomb_plan(X, [0, 2, 3], [0, 1, 2])
    eng.ct_lincomb_plan(X, [0, 1], [3])
    snap = snapshot(C1)
    with pytest.raises(PvacError, match=EINVAL):
        eng.ct_lincomb_exec(C1, plan1, call1)
    assert untouched(C1, snap)
    # ... and the same call planned again runs
    C2, plan2, call2 = eng.ct_lincomb_plan(X, [0, 2, 3], [0, 1, 2])
    out = host(eng.ct_lincomb_exec(C2, plan2, call2))
    assert [c.nE for c in out] == [pool[0].nE + pool[1].nE, pool[2].nE]
