"""The device CSPRNG on the GPU (include/pvac_hip.h: pvac_hip_aes256_ctr, pvac_hip_drbg_*, PVAC_CHAIN_DRBG):
the keystream kernel and the generator are exact against tests/drbg_model.py (pinned to FIPS-197 and
SP 800-38A by tests/test_drbg_model.py), and ct_mul, enc_value and the chain draw from it when asked."""
import threading

import numpy as np
import pytest

import drbg_model as M
from helpers import fixture_secret, hip_batch_to_host, read_u64

pytestmark = pytest.mark.gpu

KEY_C3 = bytes(range(32))
KEY_F55 = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
CTR_F55 = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
GUARD = 0x6A5D39C1E2B4F807
SEED = bytes((37 * i + 11) & 0xFF for i in range(48))
SEED2 = bytes((91 * i + 5) & 0xFF for i in range(48))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(eng.device)


def _layers(eng, X):
    """the used layer records of X, field by field (the pad word is not part of a cipher)"""
    from pvac_hfhe_cppbyv_amd import LAYER_DT
    a = np.ascontiguousarray(eng.pack(X).layers.cpu().numpy()).view(LAYER_DT).reshape(-1)
    return np.stack([a[f].astype(np.uint64) for f in ("rule", "pa", "pb", "ztag", "nonce_lo", "nonce_hi")])


def _keystream(eng, key, ctr, n, offset):
    """n words written at `offset` words from a 16-byte boundary, a guard word before and after."""
    import torch
    buf = torch.full((n + 4,), GUARD, dtype=torch.int64, device=eng.device)
    assert buf.data_ptr() % 16 == 0
    lo = 2 + offset   # words 2 (aligned) or 3 (8 mod 16)
    eng.aes256_ctr(key, ctr, n, out=buf[lo:])
    h = _u64(buf)
    assert (h[:lo] == GUARD).all() and (h[lo + n:] == GUARD).all(), "a store outside out[0, n)"
    return h[lo:lo + n]


def test_aes256_ctr_vectors_and_sizes(engine):
    eng = engine
    T, G = eng.drbg_tile()
    assert T >= 2 and G >= 1
    w = _keystream(eng, KEY_F55, CTR_F55, 8, 0)
    assert int(w[0]) == 0x33161759F17DDF0B and int(w[1]) == 0x02C560C8158B9A5E
    assert w.astype("<u8").tobytes().hex() == ("0bdf7df1591716335e9a8b15c860c5025a6e699d536119065433863c8f657b94"
                                               "1bc12c9c01610d5d0d8bd6a3378eca622956e1c8693536b1bee99c73a31576b6")
    c3 = _keystream(eng, KEY_C3, bytes.fromhex("00112233445566778899aabbccddeeff"), 2, 0)
    assert c3.astype("<u8").tobytes().hex() == "8ea2b7ca516745bfeafc49904b496089"
    big = 2 * (3 * G * T) + 1   # three grid-stride passes with a ragged end
    ref = M.ctr_words(KEY_F55, CTR_F55, big)
    for n in (0, 1, 2, 3, 2 * T - 1, 2 * T, 2 * T + 1, big):
        for offset in (0, 1):   # 16-byte stores, and out one word off a 16-byte boundary
            assert np.array_equal(_keystream(eng, KEY_F55, CTR_F55, n, offset), ref[:n]), (n, offset)


def test_aes256_ctr_carries(engine):
    eng = engine
    cases = [(((0x0123456789ABCDEF << 64) | (2**64 - 3)), 16),   # the low half wraps into the high half
             ((1 << 128) - 2, 8),                                 # the whole counter wraps
             (((0xA1B2C3D4E5F60718 << 64) | 0x293A4BFFFFFFFFFF), 6)]   # a carry through five ff bytes
    for ctr, n in cases:
        b = ctr.to_bytes(16, "big")
        for offset in (0, 1):
            assert np.array_equal(_keystream(eng, KEY_C3, b, n, offset), M.ctr_words(KEY_C3, ctr, n)), (hex(ctr), offset)


def _engine(tag=0xD5B6):
    from pvac_hfhe_cppbyv_amd import Engine
    return Engine(device=0, canon_tag=tag)


def test_drbg_fill_under_an_explicit_seed():
    import torch
    a, b = _engine(), _engine()
    a.drbg_seed(SEED)
    b.drbg_seed(SEED)
    g = M.CtrDrbg(SEED)
    assert a.drbg_counts() == (0, 0, 0, 0)
    for n in (5, 0, 1, 4097):
        t = torch.full((n + 1,), -1, dtype=torch.int64, device=a.device)
        a.drbg_fill(t[:n])
        want = g.generate(n)
        assert np.array_equal(_u64(t)[:n], want), n
        assert int(t[n].item()) == -1
        assert a.drbg_counts() == g.counts()
        u = torch.empty(max(n, 1), dtype=torch.int64, device=b.device)
        b.drbg_fill(u[:n])
        assert np.array_equal(_u64(u)[:n], want), "two contexts with one seed give one stream"
    e = bytes(range(200, 248))
    a.drbg_reseed(e)
    g.reseed(e)
    t = torch.empty(33, dtype=torch.int64, device=a.device)
    assert np.array_equal(_u64(a.drbg_fill(t)), g.generate(33))
    assert a.drbg_counts() == g.counts() == (4, 3 + 1 + 2049 + 17, 1, 0)
    # two fills enqueued back to back never share a counter
    t2 = torch.empty(2, 64, dtype=torch.int64, device=a.device)
    a.drbg_fill(t2[0])
    a.drbg_fill(t2[1])
    assert np.array_equal(_u64(t2[0]), g.generate(64)) and np.array_equal(_u64(t2[1]), g.generate(64))


def test_self_seeded_contexts_differ():
    import torch
    from pvac_hfhe_cppbyv_amd import PvacError
    a, b = _engine(), _engine()
    x = _u64(a.drbg_fill(torch.empty(8, dtype=torch.int64, device=a.device)))
    y = _u64(b.drbg_fill(torch.empty(8, dtype=torch.int64, device=b.device)))
    assert not np.array_equal(x, y) and len(set(x.tolist())) == 8
    assert a.drbg_counts() == (1, 4, 0, 1)
    with pytest.raises(PvacError):
        a._check(a.lib.pvac_hip_drbg_fill(a.ctx, None, 4))   # a null out with n > 0


def test_ct_mul_secure_draws_its_nonces_and_salts_from_the_generator():
    from pvac_hfhe_cppbyv_amd import MUL_WITH_SIGMA
    eng = _engine()
    eng.gen_H()
    A, B = eng.gen_fresh(64, 21, 20), eng.gen_fresh(64, 22, 20)
    eng.drbg_seed(SEED)
    g = M.CtrDrbg(SEED)
    C1 = eng.ct_mul(A, B, secure=True)
    _, plan = eng.ct_mul_plan(A, B)
    R1 = eng.ct_mul(A, B, nonces=_dev(eng, g.generate(2 * plan.total_layer_slots)))
    assert np.array_equal(_u64(eng.digest(C1)), _u64(eng.digest(R1)))
    assert np.array_equal(_layers(eng, C1), _layers(eng, R1))
    C2 = eng.ct_mul(A, B, secure=True)   # the generator has moved on
    g.generate(2 * plan.total_layer_slots)
    assert not np.array_equal(_layers(eng, C2), _layers(eng, C1))   # (a digest covers edges, which carry no nonce)
    # with sigma: nonces, then one salt per edge slot
    A4, B4 = eng.gen_fresh(4, 23, 20), eng.gen_fresh(4, 24, 20)
    S1 = eng.ct_mul(A4, B4, flags=MUL_WITH_SIGMA, secure=True)
    _, p4 = eng.ct_mul_plan(A4, B4)
    nz, sl = g.generate(2 * p4.total_layer_slots), g.generate(p4.total_edge_slots)
    S2 = eng.ct_mul(A4, B4, nonces=_dev(eng, nz), salts=_dev(eng, sl), flags=MUL_WITH_SIGMA)
    assert np.array_equal(_u64(eng.digest(S1)), _u64(eng.digest(S2)))
    h1, h2 = eng.pack(S1), eng.pack(S2)
    ne = int(h1.e_cnt.sum().item())
    assert ne > 0 and np.array_equal(_u64(h1.sigma[:ne]), _u64(h2.sigma[:ne]))
    assert eng.drbg_counts() == g.counts()


def _keyed_engine():
    sk, man, em = fixture_secret()
    eng = _engine(man["canon_tag"])
    assert eng.gen_H().hex() == man["H_digest"]
    eng.set_secret(read_u64("sk_prf_k.u64"), read_u64("sk_lpn_s.u64"), em["lpn_n"], em["lpn_t"], em["lpn_tau_num"],
                   em["lpn_tau_den"])
    eng.set_powg(read_u64("powg_B.u64"))
    return eng


def test_enc_value_draws_from_the_generator():
    eng = _keyed_engine()
    vals = np.random.default_rng(9).integers(0, 2**64, 16, dtype=np.uint64)
    X, st = eng.enc_value(vals)   # rnd=None
    assert not st.any()
    got, dst = eng.dec_value(X, eng.base_R(X))
    assert not dst.any() and got == [int(v) for v in vals]
    assert eng.drbg_counts()[0] == 1 and eng.drbg_counts()[3] == 1
    Y, _ = eng.enc_value(vals)
    assert not np.array_equal(_u64(eng.digest(X)), _u64(eng.digest(Y)))   # fresh draws per call


def _chain(eng, X, depth, **kw):
    """ct_mul_chain with every final cipher kept: (statistics, ciphers in input order)"""
    from pvac_hfhe_cppbyv_amd import ON_CHUNK_CB
    finals, lock = {}, threading.Lock()

    def keep(user, first, cb, stream):
        cs = hip_batch_to_host(cb.contents, stream)
        with lock:
            for i, c in enumerate(cs):
                finals[first + i] = c
        return 0

    r = eng.ct_mul_chain(X, depth, digest_n=X.n, on_chunk=ON_CHUNK_CB(keep), **kw)
    assert sorted(finals) == list(range(X.n))
    return r, [finals[i] for i in range(X.n)]


def _prod_nonces(cs):
    prod = np.concatenate([c.layers[c.layers["rule"] != 0] for c in cs])
    return np.stack([prod["nonce_lo"], prod["nonce_hi"]], axis=1)


def test_chain_with_the_generator():
    """A digest (pvac_hip_batch_digest) covers the edges, and a ct_mul's weights do not depend on its
    nonces: the digests of a chain are the same under every seed. What a seed decides are the PROD-layer
    nonces, so reproducibility and the effect of another seed are asserted on those (and the digests,
    equal throughout, on top)."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch, HostCipher
    n, depth = 8, 3
    rnd = np.random.default_rng(0xC4A1).integers(0, 2**64, (n, 256), dtype=np.uint64)
    eng = _keyed_engine()
    X, st = eng.enc_value(np.full(n, 2, np.uint64), rnd)
    assert not st.any()
    r, cs = _chain(eng, X, depth, streams=2, chunk=3, secure=True, check_gsum=True)
    assert r["gsum_pairs"] == n * depth and r["gsum_failed"] == 0
    F = DeviceBatch.from_host([HostCipher(c.layers, c.meta, c.w_lo, c.w_hi, None) for c in cs], eng.device)
    vals, dst = eng.dec_value(F, eng.base_R(F))
    assert not dst.any() and vals == [16] * n
    nz = _prod_nonces(cs)
    assert len(nz) > 0 and len({(int(a), int(b)) for a, b in nz}) == len(nz), "a PROD-layer nonce drawn twice"
    # streams = 1 under an explicit seed is reproducible on fresh engines; another seed is another run
    runs = []
    for seed in (SEED, SEED, SEED2):
        e = _keyed_engine()
        Xe, _ = e.enc_value(np.full(n, 2, np.uint64), rnd)
        e.drbg_seed(seed)
        runs.append(_chain(e, Xe, depth, streams=1, chunk=3, secure=True))
    (r0, c0), (r1, c1), (r2, c2) = runs
    assert np.array_equal(r0["digests"], r1["digests"]) and np.array_equal(_prod_nonces(c0), _prod_nonces(c1))
    assert not np.array_equal(_prod_nonces(c0), _prod_nonces(c2))
    assert not np.array_equal(_prod_nonces(c0), nz)
    # without the flag the chain is the splitmix one of nonce_seed, as before: the step-by-step run of that rule
    plain, pc = _chain(eng, X, depth, streams=2, chunk=3, nonce_seed=0x7E57)
    dig, lay = [], []
    for c0_ in range(0, n, 3):
        k = min(3, n - c0_)
        Xv = DeviceBatch(k, X.l_off[c0_:c0_ + k], X.l_cnt[c0_:c0_ + k], X.layers, X.e_off[c0_:c0_ + k],
                         X.e_cnt[c0_:c0_ + k], X.meta, X.w_lo, X.w_hi)
        cur = Xv
        for d in range(depth):
            Cb, plan = eng.ct_mul_plan(cur, Xv)
            nonces = torch.empty(2 * max(plan.total_layer_slots, 1), dtype=torch.int64, device=eng.device)
            eng.fill_random(nonces, 0x7E57 + 97 * c0_ + d)
            cur = eng.ct_mul(cur, Xv, nonces=nonces, C_=Cb, plan=plan)
        dig.append(_u64(eng.digest(cur)).copy())
        lay.append(_layers(eng, cur)[4:6])
    assert np.array_equal(plain["digests"], np.concatenate(dig))
    want = np.concatenate(lay, axis=1)
    got = np.concatenate([np.stack([c.layers["nonce_lo"], c.layers["nonce_hi"]]) for c in pc], axis=1)
    assert np.array_equal(got, want), "the default chain's nonces are no longer splitmix by nonce_seed"
