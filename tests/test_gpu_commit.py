"""GPU parity of the batched commit_ct (k_commit.hip, csrc/commit_msg.hpp): the reference-minted
digests of the fixture files, and the CPU oracle's commit_ct (oracle/pvac_oracle.cpp, the reference's
ops/commit.hpp:12-88 restated) over the shapes at which block assembly, padding, field widths, sigma
widths, capacity-padded offsets and the dealing of ciphers to lanes can go wrong."""
import ctypes as C

import numpy as np
import pytest

from commit_cases import fixture_cases
from helpers import LAYER_DT, Cipher, OrcCipher, OrcParams, _p, default_params, read_ct

pytestmark = pytest.mark.gpu

CANON = 0x5EED0C17
HD = bytes(range(7, 39))


@pytest.fixture(scope="module")
def eng():
    """A context with the digest given (set_H_digest), m_bits = 8192."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pvac_hfhe_cppbyv_amd import Engine
    e = Engine(device=0, canon_tag=CANON)
    e.set_H_digest(HD)
    return e


def orc_commit(oracle, c, canon, Hd, m_bits=8192, words=128, with_sigma=True):
    """The oracle's commit_ct with the same Params (m_bits) and row stride; with_sigma=False: nbits = 0."""
    prm = default_params(canon)
    prm.m_bits = m_bits
    sg = c.sigma if with_sigma else None
    v = OrcCipher(nL=c.nL, nE=c.nE, capL=c.nL, capE=c.nE, layers=_p(c.layers), meta=_p(c.meta), w_lo=_p(c.w_lo),
                  w_hi=_p(c.w_hi), sigma=_p(sg), sigma_words=words)
    out = C.create_string_buffer(32)
    oracle.lib.orc_commit_ct(C.byref(prm), Hd, C.byref(v), out)
    return out.raw


def rand_cipher(rng, nL, nE, prod_every=0, words=0):
    """Random fields over their whole widths: layer_id above 2^16, idx up to 65,535, ch 0 / 1, w_hi with
    bit 63 set on every other edge (the 2^63 - 1 mask applies), PROD layers at every prod_every-th slot."""
    L = np.zeros(nL, LAYER_DT)
    for f in ("ztag", "nonce_lo", "nonce_hi"):
        L[f] = rng.integers(0, 2**64, nL, dtype=np.uint64)
    L["pa"] = rng.integers(0, 2**32, nL, dtype=np.uint64)
    L["pb"] = rng.integers(0, 2**32, nL, dtype=np.uint64)
    L["pad"] = 0xFFFFFFFF   # not hashed
    if prod_every:
        L["rule"][prod_every - 1::prod_every] = 1
    lid = rng.integers(2**16, 2**32, nE, dtype=np.uint64)
    idx = rng.integers(0, 2**16, nE, dtype=np.uint64)
    idx[::3] = 65535
    ch = rng.integers(0, 2, nE, dtype=np.uint64)
    meta = lid | (idx << np.uint64(32)) | (ch << np.uint64(48))
    w_hi = rng.integers(0, 2**64, nE, dtype=np.uint64)
    w_hi[1::2] |= np.uint64(1 << 63)
    w_hi[::2] &= np.uint64((1 << 63) - 1)
    sg = rng.integers(0, 2**64, (nE, words), dtype=np.uint64) if words else None
    return Cipher(L, meta, rng.integers(0, 2**64, nE, dtype=np.uint64), w_hi, sg)


def dev_batch(engine, ciphers, words=0, pad=0):
    """Device batch, `pad` unused slots of 0xFF.. in front of every cipher's rows (capacity-padded CSR);
    words: sigma row stride (0 = no sigma array; a cipher without sigma gets zero rows)."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    n = len(ciphers)
    lc = np.array([c.nL for c in ciphers], np.uint64)
    ec = np.array([c.nE for c in ciphers], np.uint64)
    lo = (np.cumsum(lc + np.uint64(pad)) - lc).astype(np.uint64)
    eo = (np.cumsum(ec + np.uint64(pad)) - ec).astype(np.uint64)
    nl, ne = max(int((lc + np.uint64(pad)).sum()), 1), max(int((ec + np.uint64(pad)).sum()), 1)
    layers = np.zeros(nl, LAYER_DT)
    layers.view(np.uint8)[:] = 0xFF
    meta = np.full(ne, 2**64 - 1, np.uint64)
    wlo, whi = meta.copy(), meta.copy()
    sg = np.full((ne, words), 2**64 - 1, np.uint64) if words else None
    for i, c in enumerate(ciphers):
        a, b = int(lo[i]), int(eo[i])
        layers[a:a + c.nL] = c.layers
        meta[b:b + c.nE], wlo[b:b + c.nE], whi[b:b + c.nE] = c.meta, c.w_lo, c.w_hi
        if words:
            sg[b:b + c.nE] = 0 if c.sigma is None else c.sigma
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(engine.device)
    z = np.zeros(1, np.uint64)
    return DeviceBatch(n, dev(lo if n else z), dev(lc if n else z), dev(layers.view(np.int64).reshape(-1, 5)),
                       dev(eo if n else z), dev(ec if n else z), dev(meta), dev(wlo), dev(whi),
                       dev(sg) if words else None)


def hexes(d):
    return [bytes(r).hex() for r in d]


def test_golden(oracle):
    """Every fixture file a reference digest pins, as one mixed batch with sigma; the weights-only file
    through a second call with a null sigma."""
    from pvac_hfhe_cppbyv_amd import Engine
    man, cases = fixture_cases()
    e = Engine(device=0, canon_tag=man["canon_tag"])
    e.set_H_digest(bytes.fromhex(man["H_digest"]))
    cs = [read_ct(path)[0] for path, _, _ in cases]
    X = dev_batch(e, cs, words=128)
    got = hexes(e.commit_ct(X))
    got_w = hexes(e.commit_ct(X, with_sigma=False))
    assert sum(sig for _, sig, _ in cases) == 23 and len(cases) == 24
    for i, (path, sig, want) in enumerate(cases):
        assert (got if sig else got_w)[i] == want, path
        # and the other form of every file against the oracle
        Hd = bytes.fromhex(man["H_digest"])
        assert got_w[i] == orc_commit(oracle, cs[i], man["canon_tag"], Hd, with_sigma=False).hex(), path


def sweep_ciphers():
    """130 ciphers: the empty one (55 bytes: the padding exactly fills one block), one BASE layer and
    e = 0..63 edges (80 + 33 e bytes: every residue modulo 64; e = 40 is 56 modulo 64, where the length
    spills into a block of its own), and 65 with 2..8 layers, PROD layers mixed in."""
    rng = np.random.default_rng(20)
    cs = [rand_cipher(rng, 0, 0)]
    cs += [rand_cipher(rng, 1, e) for e in range(64)]
    cs += [rand_cipher(rng, 2 + e % 7, e % 64, prod_every=2 + e % 3) for e in range(65)]
    assert len(cs) == 130 and (80 + 33 * 40) % 64 == 56
    assert {(80 + 33 * e) % 64 for e in range(64)} == set(range(64))
    return cs


def test_length_sweep(eng, oracle):
    cs = sweep_ciphers()
    want = [orc_commit(oracle, c, CANON, HD, with_sigma=False).hex() for c in cs]
    assert hexes(eng.commit_ct(dev_batch(eng, cs))) == want            # two full waves and a remainder
    assert hexes(eng.commit_ct(dev_batch(eng, cs, pad=3))) == want     # the same rows behind gaps
    for i in (0, 1, 41, 64, 70, 129):                                  # n = 1: 55 bytes, 80, 56 mod 64, PROD
        assert hexes(eng.commit_ct(dev_batch(eng, [cs[i]]))) == [want[i]], i
    assert eng.commit_ct(dev_batch(eng, [])).shape == (0, 32)


def test_more_ciphers_than_lanes(eng, oracle):
    """Past 16 waves of 64 lanes on every CU the lanes that finish take further ciphers from the
    counter: 17 x 64 ciphers per CU, every one a view of one of the sweep's 130 row ranges."""
    import torch
    from pvac_hfhe_cppbyv_amd import DeviceBatch
    cs = sweep_ciphers()
    want = np.array([orc_commit(oracle, c, CANON, HD, with_sigma=False).hex() for c in cs])
    X = dev_batch(eng, cs, pad=1)
    n = 17 * 64 * torch.cuda.get_device_properties(eng.device).multi_processor_count
    pick = torch.from_numpy(np.random.default_rng(23).integers(0, len(cs), n)).to(eng.device)
    V = DeviceBatch(n, X.l_off[pick].contiguous(), X.l_cnt[pick].contiguous(), X.layers, X.e_off[pick].contiguous(),
                    X.e_cnt[pick].contiguous(), X.meta, X.w_lo, X.w_hi)
    got = eng.commit_ct(V)
    assert got.shape == (n, 32)
    first = {}
    for i, k in enumerate(pick.cpu().numpy()[:4096]):   # every sweep cipher's digest, as bytes
        first.setdefault(int(k), bytes(got[i]).hex())
    assert len(first) == len(cs) and all(first[k] == want[k] for k in first)
    table = np.stack([np.frombuffer(bytes.fromhex(w), np.uint8) for w in want])
    assert np.array_equal(got, table[pick.cpu().numpy()])


def test_fields(eng, oracle):
    """w_hi with bit 63 set (masked), layer_id above 2^16, idx 65,535, ch 0 / 1, meta bits 56-63 ignored."""
    rng = np.random.default_rng(21)
    c = rand_cipher(rng, 3, 24, prod_every=2)
    assert (c.w_hi >> np.uint64(63)).any() and (c.layer_id() > 2**16).all() and (c.idx() == 65535).any()
    assert set(c.ch().tolist()) == {0, 1}
    want = orc_commit(oracle, c, CANON, HD, with_sigma=False).hex()
    assert hexes(eng.commit_ct(dev_batch(eng, [c]))) == [want]
    m = Cipher(c.layers, c.meta, c.w_lo, c.w_hi & np.uint64(2**63 - 1))
    assert hexes(eng.commit_ct(dev_batch(eng, [m]))) == [want]          # the mask is the only use of bit 63
    hi = Cipher(c.layers, c.meta | np.uint64(0xA5 << 56), c.w_lo, c.w_hi)
    assert hexes(eng.commit_ct(dev_batch(eng, [hi]))) == [want]
    # every hashed field matters: flipping one bit of each changes the digest
    for f, bit in (("meta", 0), ("meta", 47), ("meta", 48), ("w_lo", 63), ("w_hi", 62)):
        d = Cipher(c.layers, c.meta.copy(), c.w_lo.copy(), c.w_hi.copy())
        getattr(d, f)[23] ^= np.uint64(1 << bit)
        assert hexes(eng.commit_ct(dev_batch(eng, [d]))) == [orc_commit(oracle, d, CANON, HD, with_sigma=False).hex()]
        assert hexes(eng.commit_ct(dev_batch(eng, [d]))) != [want], (f, bit)


@pytest.mark.parametrize("m_bits,words", [(8192, 128), (8192, 130), (8200, 129), (100, 2)])
def test_sigma_widths(oracle, m_bits, words):
    """Whole rows at two strides, a partial last word (8,200 bits) and a partial last byte (100 bits);
    two to five edges per cipher; the top bits of the last byte are hashed as stored."""
    from pvac_hfhe_cppbyv_amd import Engine
    e = Engine(device=0, canon_tag=CANON, m_bits=m_bits)
    e.set_H_digest(HD)
    rng = np.random.default_rng(m_bits + words)
    cs = [rand_cipher(rng, 1 + k % 2, 2 + k % 4, words=words) for k in range(9)]
    X = dev_batch(e, cs, words=words, pad=1)
    want = [orc_commit(oracle, c, CANON, HD, m_bits, words).hex() for c in cs]
    assert hexes(e.commit_ct(X)) == want
    want_w = [orc_commit(oracle, c, CANON, HD, m_bits, words, with_sigma=False).hex() for c in cs]
    assert hexes(e.commit_ct(X, with_sigma=False)) == want_w and want_w != want


def test_padded_csr_and_ragged(oracle):
    """64 fresh x fresh products with sigma committed in place from ct_mul's capacity-padded output;
    then interleaved with fresh 40-edge ciphers and empty ones, forwards and in reversed order."""
    import torch
    from pvac_hfhe_cppbyv_amd import MUL_WITH_SIGMA, Engine
    e = Engine(device=0, canon_tag=0x5EED)
    Hd = e.gen_H()
    A, B = e.gen_fresh(64, 31, 20), e.gen_fresh(64, 32, 20)
    Cb, plan = e.ct_mul_plan(A, B)
    salts = e.fill_random(torch.empty(max(plan.total_edge_slots, 1), dtype=torch.int64, device=e.device), 33)
    P = e.ct_mul(A, B, salts=salts, flags=MUL_WITH_SIGMA, C_=Cb, plan=plan, nonce_seed=34)
    assert int(P.e_off[1]) > int(P.e_cnt[0])   # capacity-padded: gaps between the ciphers
    got = hexes(e.commit_ct(P))
    hp = [Cipher(c.layers, c.meta, c.w_lo, c.w_hi, c.sigma) for c in P.to_host()]
    want = [orc_commit(oracle, c, 0x5EED, Hd).hex() for c in hp]
    assert got == want
    rng = np.random.default_rng(35)
    fresh = [Cipher(c.layers, c.meta, c.w_lo, c.w_hi, rng.integers(0, 2**64, (c.nE, 128), dtype=np.uint64))
             for c in A.to_host()[:64]]
    assert fresh[0].nE == 40
    fw = [orc_commit(oracle, c, 0x5EED, Hd).hex() for c in fresh]
    empty = Cipher(np.zeros(0, LAYER_DT), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64),
                   np.zeros((0, 128), np.uint64))
    ew = orc_commit(oracle, empty, 0x5EED, Hd).hex()
    mix, mw = [], []
    for i in range(64):
        mix += [hp[i], fresh[i], empty]
        mw += [want[i], fw[i], ew]
    assert hexes(e.commit_ct(dev_batch(e, mix, words=128, pad=2))) == mw
    assert hexes(e.commit_ct(dev_batch(e, mix[::-1], words=128, pad=2))) == mw[::-1]


def test_errors(eng, oracle):
    from pvac_hfhe_cppbyv_amd import Engine, PvacError
    rng = np.random.default_rng(22)
    c = rand_cipher(rng, 2, 5, words=128)
    bare = Engine(device=0, canon_tag=CANON)   # no gen_H, set_H or set_H_digest
    with pytest.raises(PvacError, match=r"-22.*H_digest"):
        bare.commit_ct(dev_batch(bare, [c], words=128))
    # a null sigma is the weights-only commitment, not an error
    assert hexes(eng.commit_ct(dev_batch(eng, [c]))) == [orc_commit(oracle, c, CANON, HD, with_sigma=False).hex()]
    # rows shorter than m_bits
    with pytest.raises(PvacError, match=r"-22.*shorter than m_bits"):
        eng.commit_ct(dev_batch(eng, [rand_cipher(rng, 1, 2, words=127)], words=127))
