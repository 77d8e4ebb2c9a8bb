"""GPU parity of the metrics of utils/metrics.hpp (k_metrics.hip): pvac_hip_sigma_bytehist against
np.bincount over the first ceil(m_bits / 64) words of the used sigma rows viewed as bytes, and
pvac_hip_layer_gsum against gsum_model.layer_gsums (exact) and layer_gsums_chain (the literal reference
chain, small ciphers). metrics_path_counts proves every route of both ran."""
import math
import os

import numpy as np
import pytest

import gsum_model as gm
from helpers import GOLD, LAYER_DT, P, REF, Cipher, pack_meta, read_ct
from test_gpu_add_merge import _mk
from test_gpu_recrypt import _padded_batch, _sigma_rows

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
POP8 = np.array([bin(b).count("1") for b in range(256)], np.uint64)


def _mw(m_bits):
    return (m_bits + 63) // 64


def _engine(m_bits=8192, **kw):
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, m_bits=m_bits, **kw)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _hist_model(sigma, mw):
    """The model of every histogram test: bincount over the first mw words of the rows, as bytes."""
    rows = np.ascontiguousarray(np.asarray(sigma, np.uint64)[:, :mw])
    return np.bincount(rows.reshape(-1).view(np.uint8), minlength=256).astype(np.uint64)


def _shannon(freq):
    """The reference's expression (utils/metrics.hpp:58-67), restated."""
    total = sum(int(f) for f in freq)
    if total == 0:
        return 0.0
    H = 0.0
    for f in freq:
        if int(f) > 0:
            p = float(int(f)) / total
            H -= p * math.log2(p)
    return H


def _sigma_batch(eng, e_off, e_cnt, sigma):
    """A batch of which only the counts and the sigma rows matter (the histogram reads nothing else)."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    n = len(e_cnt)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64)).to(eng.device)
    z = torch.zeros(max(n, 1), dtype=torch.int64, device=eng.device)
    return DeviceBatch(n, z, z.clone(), torch.zeros((1, 5), dtype=torch.int64, device=eng.device), dev(e_off), dev(e_cnt),
                       z.clone(), z.clone(), z.clone(), sigma)


# ------------------------------------------------------------------------------ histogram
@pytest.mark.parametrize("m_bits,words,misalign,path", [(8192, 128, False, "hist_wide"), (8192, 128, True, "hist_strided"),
                                                        (320, 5, False, "hist_strided"), (200, 6, False, "hist_strided")])
def test_bytehist_basic(m_bits, words, misalign, path):
    """0 / 1 / 63 / 64 / 65 / 513 edges in one capacity-padded batch whose unused slots are all ones;
    an aligned 128-word array takes the 16-byte path, the others (8 bytes off a 16-byte boundary, 5 words
    per row, a 6-word stride over 4 used words with a partial last word) the 8-byte path."""
    rng = np.random.default_rng(11 + m_bits)
    eng = _engine(m_bits)
    mw = _mw(m_bits)
    cs = []
    for i, ne in enumerate((0, 1, 63, 64, 65, 513)):
        c = _mk(rng, 2, ne)
        sg = np.full((c.nE, words), M64, np.uint64)   # words past mw of a row: all ones, never counted
        sg[:, :mw] = _sigma_rows(rng, c.nE, m_bits, first=i)
        cs.append(Cipher(c.layers, c.meta, c.w_lo, c.w_hi, sg))
    X = _padded_batch(eng, cs, words, misalign=misalign)
    before = eng.metrics_path_counts()
    got = _u64(eng.sigma_bytehist(X))
    assert got.shape == (len(cs), 256)
    want = np.stack([_hist_model(c.sigma, mw) for c in cs])
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=1), np.array([8 * mw * c.nE for c in cs], np.uint64))
    ones = _u64(eng.sigma_popcount(X))
    assert np.array_equal((got * POP8).sum(axis=1), ones)
    after = eng.metrics_path_counts()
    other = "hist_strided" if path == "hist_wide" else "hist_wide"
    assert after[path] == before[path] + 1 and after[other] == before[other]


def test_bytehist_constant_rows():
    """20,000 rows of 0x00 bytes and 20,000 rows of 0xA5 bytes: one share each inside a batch of 8 x CU
    count ciphers (more than 65,535 identical bytes per lane of the workgroup, 20 rounds of counters),
    then as a batch of two (1,024 shares each, flushed with atomics)."""
    import torch
    eng = _engine()
    rows, mw = 20000, 128
    a5 = int(np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0])
    sigma = torch.zeros((2 * rows, mw), dtype=torch.int64, device=eng.device)
    sigma[rows:] = a5
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 8 * cus
    want2 = np.zeros((2, 256), np.uint64)
    want2[0, 0x00] = want2[1, 0xA5] = 8 * mw * rows
    e_off, e_cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    at = (n // 3, n - 2)
    e_cnt[at[0]] = e_cnt[at[1]] = rows
    e_off[at[1]] = rows
    got = _u64(eng.sigma_bytehist(_sigma_batch(eng, e_off, e_cnt, sigma)))
    want = np.zeros((n, 256), np.uint64)
    want[at[0]], want[at[1]] = want2
    assert np.array_equal(got, want)
    got = _u64(eng.sigma_bytehist(_sigma_batch(eng, [0, rows], [rows, rows], sigma)))
    assert np.array_equal(got, want2)
    assert eng.metrics_path_counts()["hist_wide"] == 2


def test_bytehist_ragged():
    """1,000 ciphers of 0..80 rows of random bytes and one of 40,000 rows in the middle."""
    import torch
    eng = _engine()
    rng = np.random.default_rng(23)
    cnt = rng.integers(0, 81, 1001).astype(np.uint64)
    cnt[500] = 40000
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    total = int(cnt.sum())
    sigma = torch.empty((total, 128), dtype=torch.int64, device=eng.device)
    eng.fill_random(sigma, 99)
    got = _u64(eng.sigma_bytehist(_sigma_batch(eng, off, cnt, sigma)))
    host = sigma.cpu().numpy().view(np.uint8).reshape(total, 1024)
    for i in range(len(cnt)):
        a, b = int(off[i]), int(off[i] + cnt[i])
        assert np.array_equal(got[i], np.bincount(host[a:b].reshape(-1), minlength=256).astype(np.uint64)), i


def test_bytehist_real_sigma():
    """Reference-minted ciphers with sigma: the fresh x fresh product pair0_mul.ct and ct_recrypt's
    output fresh_out.ct (recrypt/product_out.ct, the recrypted product, is stored weights-only: its
    sigmas live only in its commitment, so it cannot serve here). The histogram equals numpy's,
    Engine.sigma_shannon the restated expression on those counts exactly, and real sigma bytes are near
    uniform: the entropy lies in (7.9, 8.0] (7.9998 and 7.9953 on the fixtures' bytes, checked on the CPU
    before it is asked of the device)."""
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    eng = _engine()
    assert read_ct(os.path.join(GOLD, "recrypt", "product_out.ct"))[0].sigma is None
    cs = [read_ct(os.path.join(REF, "pair0_mul.ct"))[0], read_ct(os.path.join(GOLD, "recrypt", "fresh_out.ct"))[0]]
    want = np.stack([_hist_model(c.sigma, 128) for c in cs])
    want_H = [_shannon(w) for w in want]
    assert all(c.sigma is not None and c.nE for c in cs) and all(7.9 < h <= 8.0 for h in want_H), want_H
    X = DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in cs], eng.device, sigma=True)
    assert np.array_equal(_u64(eng.sigma_bytehist(X)), want)
    H = eng.sigma_shannon(X)
    assert H.dtype == np.float64 and [float(h) for h in H] == want_H
    assert all(7.9 < h <= 8.0 for h in H)


def test_bytehist_errors():
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch, PvacError
    eng = _engine()
    X = _sigma_batch(eng, [0], [4], None)
    with pytest.raises(PvacError, match="-22"):
        eng.sigma_bytehist(X)
    X = _sigma_batch(eng, [0], [4], torch.zeros((4, 64), dtype=torch.int64, device=eng.device))   # 64 words < 8192 bits
    with pytest.raises(PvacError, match="-22"):
        eng.sigma_bytehist(X)
    assert eng.sigma_bytehist(DeviceBatch.empty(0, 0, 0, eng.device, sigma=True)).shape == (0, 256)
    assert eng.sigma_shannon(DeviceBatch.empty(0, 0, 0, eng.device, sigma=True)).shape == (0,)
    c = eng.metrics_path_counts()
    assert c["hist_wide"] == 0 and c["hist_strided"] == 0


# ------------------------------------------------------------------------------ layer gsums
SENTINEL = np.uint64(M64)


@pytest.fixture(scope="module")
def geng():
    from pvac_hfhe_cppbyv_amd import Engine, powg_table
    eng = Engine(device=0)
    pg = powg_table()
    eng.set_powg(pg)
    return eng, pg


def _weights_batch(eng, ciphers):
    """Capacity-padded batch (an unused layer slot and three unused edge slots after every cipher, all
    ones) of ciphers whose sigma does not matter."""
    return _padded_batch(eng, [Cipher(c.layers, c.meta, c.w_lo, c.w_hi, np.zeros((c.nE, 1), np.uint64)) for c in ciphers], 1)


def _check_gsums(eng, X, ciphers, want, want_status=None):
    """want[i]: list of integers, or None to skip cipher i's sums. Slots past l_cnt keep the sentinel."""
    out, st = eng.layer_gsum(X, status=True)
    g = _u64(out)
    lo = _u64(X.l_off)
    used = np.zeros(len(g), bool)
    for i, c in enumerate(ciphers):
        a = int(lo[i])
        used[a:a + c.nL] = True
        if want[i] is None:
            continue
        got = [int(g[a + l, 0]) | (int(g[a + l, 1]) << 64) for l in range(c.nL)]
        assert got == want[i], (i, [l for l in range(c.nL) if got[l] != want[i][l]][:5])
    assert np.all(g[~used] == SENTINEL)
    assert np.array_equal(st, np.zeros(len(ciphers), np.uint32) if want_status is None else np.asarray(want_status, np.uint32))
    return g


def test_gsum_reference_ciphers(oracle, geng):
    """Reference-minted chain and product ciphers (BASE and PROD layers) with an empty and a one-edge
    cipher, capacity-padded: the exact model everywhere, the literal fp_add / fp_sub chain up to 2,000
    edges."""
    eng, pg = geng
    cs = [read_ct(os.path.join(REF, f))[0] for f in ("chain0.ct", "chain1.ct", "chain2.ct", "chain3.ct", "chainf_final.ct",
                                                     "pair0_mul.ct")]
    assert any((c.layers["rule"] == 1).any() for c in cs)
    rng = np.random.default_rng(3)
    cs += [Cipher(np.zeros(0, LAYER_DT), [], [], []), _mk(rng, 1, 1)]
    want = [gm.layer_gsums(oracle, c, pg) for c in cs]
    literal = 0
    for c, w in zip(cs, want):
        if c.nE <= 2000:
            assert [lo | (hi << 64) for lo, hi in gm.layer_gsums_chain(oracle, c, pg)] == w
            literal += 1
    assert literal >= 3
    before = eng.metrics_path_counts()
    _check_gsums(eng, _weights_batch(eng, cs), cs, want)
    after = eng.metrics_path_counts()
    moved = {k: after[k] - before[k] for k in ("gsum_wave", "gsum_workgroup", "gsum_large")}
    assert moved["gsum_wave"] >= 2 and moved["gsum_workgroup"] >= 1 and sum(moved.values()) == len(cs)


def test_gsum_of_a_product(geng):
    """ct_mul on the GPU of two 3-layer ciphers: every product layer, found by its nonce, carries
    fp_mul(gsum(A, la), gsum(B, lb))."""
    import torch
    from pvac_hfhe_cppbyv_amd import FP_MUL, DeviceBatch, HostCipher
    eng, _ = geng
    rng = np.random.default_rng(41)
    a, b = _mk(rng, 3, 60), _mk(rng, 3, 45)
    dev = lambda c: DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi)], eng.device)
    A, B = dev(a), dev(b)
    Cb, plan = eng.ct_mul_plan(A, B)
    nonces = torch.empty(2 * plan.total_layer_slots, dtype=torch.int64, device=eng.device)
    eng.fill_random(nonces, 77)
    C_ = eng.ct_mul(A, B, nonces=nonces, C_=Cb, plan=plan)
    gA, gB, gC = (_u64(eng.layer_gsum(X)) for X in (A, B, C_))
    c = C_.to_host()[0]
    nz = _u64(nonces).reshape(-1, 2)
    base = int(_u64(Cb.l_off)[0]) + 3 + 3
    slot = {(int(nz[base + q, 0]), int(nz[base + q, 1])): q for q in range(9)}
    prod = [(l, slot[(int(y["nonce_lo"]), int(y["nonce_hi"]))]) for l, y in enumerate(c.layers) if int(y["rule"]) == 1]
    assert len(prod) == 9 and c.nE > 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(eng.device)
    la, lb = [q // 3 for _, q in prod], [q % 3 for _, q in prod]
    lo, hi = eng.fp_binop(FP_MUL, t(gA[la, 0]), t(gA[la, 1]), t(gB[lb, 0]), t(gB[lb, 1]))
    lc = int(_u64(C_.l_off)[0])
    rows = [lc + l for l, _ in prod]
    assert np.array_equal(gC[rows, 0], _u64(lo)) and np.array_equal(gC[rows, 1], _u64(hi))
    assert np.any(gC[rows] != 0)


def test_gsum_contract_edges(oracle, geng):
    """Edges naming a layer past l_cnt are ignored; idx = B gives status 2 for that cipher alone;
    non-canonical weight words (w = p, w = 2^128 - 1) follow fp_mul. The neighbours' sums stand."""
    eng, pg = geng
    rng = np.random.default_rng(57)
    normal = [_mk(rng, 2 + i, 30 + 7 * i) for i in range(4)]
    stray = _mk(rng, 2, 50)
    stray.meta[::5] = pack_meta(2 + (stray.meta[::5] & np.uint64(3)), stray.idx()[::5], stray.ch()[::5])
    assert (stray.layer_id() >= 2).sum() == 10
    bad = _mk(rng, 3, 40)
    bad.meta[17] = pack_meta(1, 337, 0)
    nc = _mk(rng, 2, 24)
    nc.w_lo[::3], nc.w_hi[::3] = np.uint64(M64), np.uint64((1 << 63) - 1)    # w = p
    nc.w_lo[1::3], nc.w_hi[1::3] = np.uint64(M64), np.uint64(M64)             # w = 2^128 - 1
    cs = [normal[0], stray, normal[1], bad, normal[2], nc, normal[3]]
    want = [None if c is bad else gm.layer_gsums(oracle, c, pg) for c in cs]
    _check_gsums(eng, _weights_batch(eng, cs), cs, want, want_status=[0, 0, 0, 2, 0, 0, 0])


def _bound_cipher(eng, per_layer, views=()):
    """One cipher of 3 layers with `per_layer` edges each (layer-major), every edge idx 0 and w = p - 1:
    layer 0 all SGN_P, layer 1 all SGN_M, layer 2 alternating from SGN_P. views: further ciphers of one
    layer over its first `t` edges (all in layer 0, SGN_P)."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    d = eng.device
    k = torch.arange(per_layer, dtype=torch.int64, device=d)
    meta = torch.cat([torch.zeros_like(k), torch.full_like(k, 1 | (1 << 48)), 2 | ((k & 1) << 48)])
    ne = 3 * per_layer
    w_lo = torch.full((ne,), -2, dtype=torch.int64, device=d)              # 2^64 - 2
    w_hi = torch.full((ne,), (1 << 63) - 1, dtype=torch.int64, device=d)   # p - 1 = 2^127 - 2
    n = 1 + len(views)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=d)
    return DeviceBatch(n, t([0] + [3 + j for j in range(len(views))]), t([3] + [1] * len(views)),
                       torch.zeros((3 + len(views), 5), dtype=torch.int64, device=d), t([0] * n), t([ne] + list(views)),
                       meta, w_lo, w_hi)


@pytest.mark.parametrize("per_layer", [(1 << 21) - 1, 1 << 21, (1 << 21) + 5])
def test_gsum_beyond_the_limb_bound(geng, per_layer):
    """Limb sums of 2^21 + 1 maximal terms pass 2^64: the op sums such a cipher in pieces folded mod p.
    Every term is fp_mul(p - 1, powg_B[0] = 1) = p - 1, every limb at its maximum. Expected, from Python
    integers: layer 0 = n (p - 1), layer 1 = -n (p - 1), layer 2 = p - 1 for an odd n (the extra edge is
    SGN_P) and 0 for an even one. Next to it, one-layer ciphers over the first 2^21 - 1 and 2^21 edges
    of layer 0: the first stays on the workgroup route, from 2^21 edges on the large route runs."""
    eng, pg = geng
    assert int(pg[0]) == 1 and int(pg[1]) == 0
    views = ((1 << 21) - 1, 1 << 21) if per_layer >= 1 << 21 else ()
    X = _bound_cipher(eng, per_layer, views)
    before = eng.metrics_path_counts()
    out, st = eng.layer_gsum(X, status=True)
    after = eng.metrics_path_counts()
    g = _u64(out)
    got = [int(g[s, 0]) | (int(g[s, 1]) << 64) for s in range(len(g))]
    want = [per_layer * (P - 1) % P, -per_layer * (P - 1) % P, (per_layer % 2) * (P - 1) % P] + [t * (P - 1) % P for t in views]
    assert got == want
    assert not st.any()
    # 3 n edges in the cipher: beyond 2^21 in every case; the one-layer ciphers sit on the boundary
    assert after["gsum_large"] - before["gsum_large"] == 1 + (1 if views else 0)
    assert after["gsum_workgroup"] - before["gsum_workgroup"] == (1 if views else 0)


def test_gsum_tables_beyond_lds(oracle, geng):
    """4,000 layers are 192 KB of tables, more than a workgroup's 160 KiB of LDS: a slab of scratch."""
    eng, pg = geng
    rng = np.random.default_rng(71)
    cs = [_mk(rng, 4000, 8000), _mk(rng, 2, 40)]
    before = eng.metrics_path_counts()
    _check_gsums(eng, _weights_batch(eng, cs), cs, [gm.layer_gsums(oracle, c, pg) for c in cs])
    after = eng.metrics_path_counts()
    assert after["gsum_large"] - before["gsum_large"] == 1 and after["gsum_wave"] - before["gsum_wave"] == 1


def test_gsum_many_small_ciphers(oracle, geng):
    """gen_fresh(4096): a wave per cipher. The model runs once, over the batch read as one cipher of
    8,192 layers (layer 2 i + l of the whole is layer l of cipher i)."""
    eng, pg = geng
    n = 4096
    X = eng.gen_fresh(n, 5, 20)
    hs = X.to_host()
    assert all(h.nL == 2 and h.nE == 40 for h in hs)
    meta = np.concatenate([h.meta + np.uint64(2 * i) for i, h in enumerate(hs)])
    whole = Cipher(np.concatenate([h.layers for h in hs]), meta, np.concatenate([h.w_lo for h in hs]),
                   np.concatenate([h.w_hi for h in hs]))
    assert np.array_equal(whole.layer_id() // 2, np.repeat(np.arange(n), 40))
    want = gm.layer_gsums(oracle, whole, pg)
    before = eng.metrics_path_counts()
    out, st = eng.layer_gsum(X, status=True)
    after = eng.metrics_path_counts()
    g = _u64(out)
    assert [int(g[s, 0]) | (int(g[s, 1]) << 64) for s in range(2 * n)] == want
    assert not st.any()
    assert after["gsum_wave"] - before["gsum_wave"] == n


def test_gsum_needs_powg():
    from pvac_hfhe_cppbyv_amd import PvacError
    eng = _engine()
    with pytest.raises(PvacError, match="powg"):
        eng.layer_gsum(eng.gen_fresh(4, 1, 20))
